// What the fused loss kernels (infonce.hip, table_nce.hip, clcrec.hip, ccfcrec.hip, aldi.hip, gar.hip, mtpr.hip, vbpr.hip)
// share: the wave and lane-group sums, the lane-group coordinates, the front of the one-workgroup loss kernels, the owner
// pass that sums per-occurrence gradient rows by their owner, and on the host the workspace carver, the argument checks
// with their messages, the owners' inverse index of a plan and the dispatch on the lane-group width.
//
// A lane group is LPR = pow2(d / 4) lanes that hold one row of d floats, four columns per lane (16-byte loads); a wave
// holds 64 / LPR rows at a time.
#pragma once
#include <type_traits>

#include "crh_common.h"

namespace {

// ---- device ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float lg_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ float lg_wave_max(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

// sum over the LPR lanes of a row's group / over the 64 / LPR groups (same column of every group)
template <int LPR>
__device__ __forceinline__ float lg_group_sum(float v) {
#pragma unroll
    for (int off = LPR / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

template <int LPR>
__device__ __forceinline__ float lg_cross_sum1(float v) {
    if constexpr (LPR < 64) {                          // (one group per wave: nothing to add)
#pragma unroll
        for (int off = 32; off >= LPR; off >>= 1) v += __shfl_xor(v, off);
    }
    return v;
}

// (a caller that sits next to other LPR < 64 work keeps its own `if constexpr (LPR < 64)` around the call: hipcc 7.2
// crashes on some of the no-op calls)
template <int LPR>
__device__ __forceinline__ f32x4 lg_cross_sum(f32x4 v) {
    if constexpr (LPR < 64) {
#pragma unroll
        for (int off = 32; off >= LPR; off >>= 1) {
            const float x = __shfl_xor(v[0], off), y = __shfl_xor(v[1], off);
            const float z = __shfl_xor(v[2], off), w = __shfl_xor(v[3], off);
            v += f32x4{x, y, z, w};
        }
    }
    return v;
}

__device__ __forceinline__ f32x4 lg_load4(const float* p, bool ok) {
    return ok ? *reinterpret_cast<const f32x4*>(p) : f32x4{0.f, 0.f, 0.f, 0.f};
}

__device__ __forceinline__ float lg_dot4(const f32x4& a, const f32x4& b) {
    return (a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3]);
}

// where a lane stands: `const auto [lane, cl, grp, col] = lg_coords<LPR>();` -- the lane, its place in its group, the
// group (= the row of the pass) and the first of its four columns
struct LgCoords {
    int lane, cl, grp, col;
};
template <int LPR>
__device__ __forceinline__ LgCoords lg_coords() {
    const int lane = threadIdx.x & 63, cl = lane & (LPR - 1), grp = LPR == 64 ? 0 : lane / LPR;
    return {lane, cl, grp, 4 * cl};
}

// ---- the owner pass: per-occurrence gradient rows summed by their owner ---------------------------------------------
// gar.hip, mtpr.hip and vbpr.hip end with the two kernels below through lg_owner_pass.  ccfcrec.hip's two chunk kernels
// and clcrec.hip's do other work per occurrence (a weight, a sign, rank vectors) and stay in their files; they share
// LG_CHUNK and the plan's layout only.  (A chunk's bounds -- k_begin = ptr[s] + (ch - chunk_ptr[s]) * LG_CHUNK, k_end
// clamped to ptr[s + 1] -- are written out in every walk: as a function of any shape they changed the code generated
// around the walk that follows them.  A whole kernel moved in here compiles as it did in its file.)
constexpr int LG_CHUNK = 256;       // occurrences of one owner summed by one wave

// What an owner's summed row becomes.  With a table: + weight(n_first, n_all) x the owner's table row, written at the
// owner's row of the table's gradient; n_all = the owner's occurrences, n_first = those below `first` (counted by the
// chunk kernel for a COUNT_FIRST finish only).  Without one: the sum as it stands at row s.
struct LgFinishReg {                // an L2 term per occurrence: reg2 n_all (MTPR, VBPR)
    static constexpr bool TABLE = true, COUNT_FIRST = false;
    float reg2;
    __device__ float weight(int64_t, int64_t n_all) const { return reg2 * (float)n_all; }
};
struct LgFinishNorms {              // a block-norm term, one block up to `first` and one after it (GAR)
    static constexpr bool TABLE = true, COUNT_FIRST = true;
    const float* rinv;
    int r_first, r_second;
    __device__ float weight(int64_t n_first, int64_t n_all) const {
        return (float)n_first * rinv[r_first] + (float)(n_all - n_first) * rinv[r_second];
    }
};
struct LgFinishSum {                // VBPR's hsum
    static constexpr bool TABLE = false, COUNT_FIRST = false;
};

// One wave per chunk of one owner's occurrences: occurrence o takes row o of `rows` (d floats).  part[chunk] = d floats
// -- with COUNT_FIRST d + 4: the sum, then the chunk's count of o < first as an integer's bits.
// (offsets and occurrences are read as unsigned: an item side's run to 2 B < 2^32)
template <int LPR, bool COUNT_FIRST>
__global__ __launch_bounds__(64) void lg_owner_chunk_kernel(const uint32_t* __restrict__ own_ptr,
                                                            const uint32_t* __restrict__ own_rows,
                                                            const int32_t* __restrict__ chunk_ptr,
                                                            const int32_t* __restrict__ chunk_own, int64_t n_own,
                                                            int64_t occurrences, int d, const float* __restrict__ rows,
                                                            float* __restrict__ part, int64_t first) {
    constexpr int RG = 64 / LPR;
    const int64_t ch = blockIdx.x;
    const auto [lane, cl, grp, col] = lg_coords<LPR>();
    const bool ok = col < d;
    const int s = chunk_own[ch];
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    [[maybe_unused]] int n_first = 0;
    if (s >= 0 && s < n_own) {                          // (uniform: a malformed plan sums nothing instead of reading wild)
        const int64_t k_begin = (int64_t)own_ptr[s] + (ch - chunk_ptr[s]) * LG_CHUNK;
        int64_t k_end = k_begin + LG_CHUNK;
        if (k_end > own_ptr[s + 1]) k_end = own_ptr[s + 1];
        if (k_end > occurrences) k_end = occurrences;
        for (int64_t k0 = k_begin; k0 < k_end; k0 += 64) {
            const bool have = k0 + lane < k_end;
            const uint32_t mine = have ? own_rows[k0 + lane] : 0u;
#pragma unroll 4
            for (int j = 0; j < LPR; ++j) {
                const int src = j * RG + grp;
                const int64_t o = __shfl(mine, src);
                if (!__shfl((int)have, src) || o >= occurrences || !ok) continue;
                acc += *reinterpret_cast<const f32x4*>(rows + o * d + col);
                if constexpr (COUNT_FIRST) n_first += o < first;
            }
        }
    }
    if constexpr (LPR < 64) {
        acc = lg_cross_sum<LPR>(acc);
        if constexpr (COUNT_FIRST) {
#pragma unroll
            for (int off = 32; off >= LPR; off >>= 1) n_first += __shfl_xor(n_first, off);
        }
    }
    if constexpr (COUNT_FIRST) {
        if (grp == 0 && ok) {
            float* p = part + ch * (d + 4);
            *reinterpret_cast<f32x4*>(p + col) = acc;
            if (cl == 0) *reinterpret_cast<f32x4*>(p + d) = f32x4{__int_as_float(n_first), 0.f, 0.f, 0.f};
        }
    } else {
        if (grp == 0 && ok) *reinterpret_cast<f32x4*>(part + ch * d + col) = acc;
    }
}

// one lane group per distinct owner: the chunks in chunk order, then the finish
template <int LPR, class Finish>
__global__ __launch_bounds__(64) void lg_owner_finish_kernel(const float* __restrict__ table, int64_t table_rows,
                                                             const int32_t* __restrict__ own_ids,
                                                             const uint32_t* __restrict__ own_ptr,
                                                             const int32_t* __restrict__ chunk_ptr, int64_t n_own, int d,
                                                             const float* __restrict__ part, const Finish fin,
                                                             float* __restrict__ out) {
    constexpr int RG = 64 / LPR;
    const auto [lane, cl, grp, col] = lg_coords<LPR>();
    const int64_t s = (int64_t)blockIdx.x * RG + grp;
    if (col >= d || s >= n_own) return;
    int64_t id = s;
    if constexpr (Finish::TABLE) {
        id = own_ids[s];
        if (id < 0 || id >= table_rows) return;
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    [[maybe_unused]] int64_t n_first = 0;
    for (int64_t ch = chunk_ptr[s]; ch < chunk_ptr[s + 1]; ++ch) {
        if constexpr (Finish::COUNT_FIRST) {
            const float* p = part + ch * (d + 4);
            acc += *reinterpret_cast<const f32x4*>(p + col);
            n_first += __float_as_int(p[d]);
        } else {
            acc += *reinterpret_cast<const f32x4*>(part + ch * d + col);
        }
    }
    if constexpr (Finish::TABLE) {
        const int64_t n_all = (int64_t)own_ptr[s + 1] - (int64_t)own_ptr[s];
        const float w = fin.weight(n_first, n_all);
        const f32x4 row = *reinterpret_cast<const f32x4*>(table + id * d + col);
        acc += row * w;
    }
    *reinterpret_cast<f32x4*>(out + id * d + col) = acc;
}

// the front of a one-workgroup loss kernel (256 threads): red[w][q] = wave w's part of sum_b rec[4 b + q], every thread its
// records in index order, then the wave; ends with the barrier.  Thread 0 then adds the waves as (0 + 1) + (2 + 3) in the
// kernel's own body (with that sum in here the compiler contracted the total of ccfcrec's epilogue differently).
__device__ __forceinline__ void lg_record_sums(const float* rec, int64_t batch, float (*red)[4]) {
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t b = threadIdx.x; b < batch; b += 256)
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] += rec[b * 4 + q];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        s[q] = lg_wave_sum(s[q]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = s[q];
    }
    __syncthreads();
}

// ---- what the two streamed-softmax kernels (infonce.hip, table_nce.hip) share ---------------------------------------
constexpr int NCE_WAVES = 4;          // waves per workgroup: 4 row blocks that share one streamed tile in LDS
constexpr float NCE_EPS = 1e-12f;     // F.normalize's clamp_min
constexpr float LN2 = 0.6931471805599453f;

__host__ __device__ inline int64_t ceil32(int64_t x) { return (x + 31) & ~(int64_t)31; }

__device__ __forceinline__ int read_n(const int32_t* n_dev, int64_t n_max) {
    if (!n_dev) return (int)n_max;
    const int n = n_dev[0];
    return n < 0 ? 0 : (n > n_max ? (int)n_max : n);
}

// row of the accumulator register r in lane half h (C/D map of the 32x32 MFMA shapes)
__device__ __forceinline__ int crow(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// ---- host -----------------------------------------------------------------------------------------------------------
// hands out 256-byte aligned float arrays of a workspace one after the other; from a NULL base it only counts the bytes
struct WsCarver {
    char* base;
    size_t bytes = 0;
    explicit WsCarver(void* b) : base(reinterpret_cast<char*>(b)) {}
    float* take(int64_t floats) {
        float* r = reinterpret_cast<float*>(base + bytes);
        bytes += (size_t)((floats * 4 + 255) & ~(int64_t)255);
        return r;
    }
};

inline bool lg_ws_ok(const char* fn, const void* workspace, size_t workspace_bytes, size_t need) {
    if (workspace && workspace_bytes >= need && !(reinterpret_cast<uintptr_t>(workspace) & 255)) return true;
    crh_set_error("%s: workspace %zu < %zu bytes (or not 256-byte aligned)", fn, workspace_bytes, need);
    return false;
}
#define LG_CHECK_WS(fn, workspace, workspace_bytes, need)                       \
    do {                                                                        \
        if (!lg_ws_ok(fn, workspace, workspace_bytes, need)) return CRH_ERR_WS; \
    } while (0)

inline bool lg_width_ok(int d) { return d >= 4 && d <= 256 && d % 4 == 0; }
#define LG_CHECK_WIDTH(fn, d) CRH_CHECK_ARG(lg_width_ok(d), "%s: d = %d must be a multiple of 4 in [4, 256]", fn, d)

// what: "user" or "item"
#define LG_CHECK_IDS(fn, what, lo, hi, rows)                                                                       \
    CRH_CHECK_ARG((lo) >= 0 && (lo) <= (hi) && (hi) < (rows), "%s: %s ids [%d, %d] outside the %s table of %lld rows", \
                  fn, what, lo, hi, what, (long long)(rows))

// One side (the users or the items) of a plan's inverse index, as ccfcrec.hip, gar.hip, mtpr.hip and vbpr.hip take it: the n
// distinct owners (ids), their occurrences grouped by owner (ptr, occ) and cut into n_chunks chunks (chunk_ptr, chunk_own).
struct LgOwners {
    const int32_t *ids, *ptr, *occ, *chunk_ptr, *chunk_own;
    int64_t n, n_chunks;
    bool complete() const { return ids && ptr && occ && chunk_ptr && chunk_own; }
};

// the most chunks that `occurrences` occurrences of n_own owners are cut into
inline int64_t lg_max_chunks(int64_t occurrences, int64_t n_own, int chunk) { return n_own + occurrences / chunk; }

// (offsets and occurrences are read as unsigned by the chunk kernels)
inline const uint32_t* lg_u32(const int32_t* p) { return reinterpret_cast<const uint32_t*>(p); }

#define LG_CHECK_OWNER_PTRS(fn, items, users) \
    CRH_CHECK_ARG((items).complete() && (users).complete(), "%s: NULL inverse-index pointer", fn)

// the owners' and the chunks' counts of both sides; *_occ = a side's occurrences, *_txt = how the messages spell them
#define LG_CHECK_OWNER_COUNTS(fn, items, item_occ, item_txt, users, user_occ, user_txt, chunk)                              \
    do {                                                                                                                    \
        CRH_CHECK_ARG((items).n >= 1 && (items).n <= (item_occ), "%s: n_items = %lld out of [1, %s]", fn,                   \
                      (long long)(items).n, item_txt);                                                                      \
        CRH_CHECK_ARG((users).n >= 1 && (users).n <= (user_occ), "%s: n_users = %lld out of [1, %s]", fn,                   \
                      (long long)(users).n, user_txt);                                                                      \
        CRH_CHECK_ARG((items).n_chunks >= (items).n && (items).n_chunks <= lg_max_chunks(item_occ, (items).n, chunk),       \
                      "%s: n_item_chunks = %lld out of [n_items, n_items + %s / %d]", fn, (long long)(items).n_chunks,      \
                      item_txt, chunk);                                                                                     \
        CRH_CHECK_ARG((users).n_chunks >= (users).n && (users).n_chunks <= lg_max_chunks(user_occ, (users).n, chunk),       \
                      "%s: n_user_chunks = %lld out of [n_users, n_users + %s / %d]", fn, (long long)(users).n_chunks,      \
                      user_txt, chunk);                                                                                     \
    } while (0)

// What crh_gar_f32, crh_mtpr_f32 and crh_vbpr_f32 check alike, in two parts: each has checks of its own in between.  A
// plan of (user, positive, negative) records has 2 batch item occurrences and batch user occurrences, cut by LG_CHUNK.
#define LG_CHECK_TRIPLE_PTRS(fn, users, pos, neg, items, owners)              \
    do {                                                                      \
        CRH_CHECK_ARG((users) && (pos) && (neg), "%s: NULL id pointer", fn);  \
        LG_CHECK_OWNER_PTRS(fn, items, owners);                               \
    } while (0)

// batch_log2: the batch lies in [1, 2^batch_log2)
#define LG_CHECK_TRIPLE_SHAPE(fn, batch, batch_log2, items, owners, user_min, user_max, user_rows, item_min, item_max,   \
                              item_rows)                                                                                 \
    do {                                                                                                                 \
        CRH_CHECK_ARG((batch) >= 1 && (batch) < ((int64_t)1 << (batch_log2)), "%s: batch = %lld must lie in [1, 2^%d)",  \
                      fn, (long long)(batch), batch_log2);                                                               \
        LG_CHECK_OWNER_COUNTS(fn, items, 2 * (batch), "2 batch", owners, batch, "batch", LG_CHUNK);                      \
        LG_CHECK_IDS(fn, "user", user_min, user_max, user_rows);                                                         \
        LG_CHECK_IDS(fn, "item", item_min, item_max, item_rows);                                                         \
    } while (0)

// the shapes whose workspace the three size: the same bounds, with the kernel's widest d
inline bool lg_triple_shape_ok(int64_t batch, int batch_log2, int d, int d_max, int64_t n_items, int64_t n_users) {
    return batch >= 1 && batch < ((int64_t)1 << batch_log2) && lg_width_ok(d) && d <= d_max && n_items >= 1 &&
           n_items <= 2 * batch && n_users >= 1 && n_users <= batch;
}

template <class... T>
inline bool lg_aligned16(const T*... p) {
    return ((reinterpret_cast<uintptr_t>(p) | ...) & 15) == 0;
}

// f(std::integral_constant<int, LPR>) with LPR = pow2(d / 4)
template <class F>
inline void lg_dispatch_lpr(int d, F&& f) {
    const int lanes = d / 4;
    if (lanes <= 1) f(std::integral_constant<int, 1>{});
    else if (lanes <= 2) f(std::integral_constant<int, 2>{});
    else if (lanes <= 4) f(std::integral_constant<int, 4>{});
    else if (lanes <= 8) f(std::integral_constant<int, 8>{});
    else if (lanes <= 16) f(std::integral_constant<int, 16>{});
    else if (lanes <= 32) f(std::integral_constant<int, 32>{});
    else f(std::integral_constant<int, 64>{});
}

// One owner pass: the rows of `rows`, one of d floats per occurrence, summed by the owners of o through `part` (a chunk's
// partial: d floats, d + 4 for a COUNT_FIRST finish, whose `first` counts then) and finished by `fin` into `out`;
// table = NULL with LgFinishSum.
template <class Finish>
inline void lg_owner_pass(const LgOwners& o, const float* table, int64_t table_rows, int64_t occurrences, int d,
                          const float* rows, float* part, const Finish& fin, float* out, hipStream_t st,
                          int64_t first = 0) {
    lg_dispatch_lpr(d, [&](auto lpr) {
        constexpr int LPR = decltype(lpr)::value, RG = 64 / LPR;
        hipLaunchKernelGGL((lg_owner_chunk_kernel<LPR, Finish::COUNT_FIRST>), dim3((unsigned)o.n_chunks), dim3(64), 0, st,
                           lg_u32(o.ptr), lg_u32(o.occ), o.chunk_ptr, o.chunk_own, o.n, occurrences, d, rows, part, first);
        hipLaunchKernelGGL((lg_owner_finish_kernel<LPR, Finish>), dim3((unsigned)((o.n + RG - 1) / RG)), dim3(64), 0, st,
                           table, table_rows, o.ids, lg_u32(o.ptr), o.chunk_ptr, o.n, d, part, fin, out);
    });
}

}  // namespace
