// Screened ranking of fp32 d=128 catalogues (the headline shape): the catalogue is walked once in fp16 by the
// LDS-DMA kernel (16x the fp32 MFMA rate) keeping K' = SCREEN_KP > k candidates per user, the candidates are rescored with the
// canonical fmaf chain, and a per-user certificate proves that no item outside them can enter the exact top-k.  Users without
// the proof are ranked exactly by the fallback below.  This file holds the kernels of stages 0 (fp16 copies and their error
// norms), 2 (rescoring + certificate) and 3 (exact fallback); score_topk.hip runs stage 1 and the orchestration.
//
// The bound.  u, v: fp32 rows; u^, v^: their fp16 copies scaled back (one power of two per table, so scaling is exact);
// a: the approximate score the fp16 kernel ranked by (its fp32 accumulator, scaled back); s: the exact fmaf chain.
//   |s - u.v|     <= g_d |u| |v|               (d-term fma chain, g_d = d 2^-24 / (1 - d 2^-24))
//   |u.v - u^.v^| <= |u| |v - v^| + |u - u^| |v^|
//   |u^.v^ - a|   <= g' |u^| |v^|              (f16 x f16 products are exact in fp32; g' = 2^-12 covers any fp32 accumulation order)
// so |s - a| <= B_u = |u| R + |u - u^| N^ + g_d |u| N + g' |u^| N^ with R = max |v - v^|, N = max |v|, N^ = max |v^| over the
// unmasked rows of the shard.  The fp16 copies carry no subnormals (flushed to zero here, which lands in the residuals), so
// every partial sum of the MFMA is a multiple of 2^-48 of the scaled operands and never underflows; the exact chain's own
// subnormal roundings are covered by an absolute term.  Norms are evaluated in fp64 and rounded up; a non-finite input makes
// its norm +inf (or NaN), and then no comparison with the bound can pass.
#include <math.h>

#include "score_topk_common.h"

#include <hipcub/device/device_radix_sort.hpp>

namespace crh_score {
namespace {

constexpr int SD = 128;            // row width of the screened route
constexpr int FB_SCRATCH_SLICES = 64;  // slice lists per user the workspace holds for the fallback (screen_fallback_slices)

// a float that is >= x (x >= 0 or NaN); +inf when x is NaN or beyond the float range
__device__ __forceinline__ float up_float(double x) {
    if (!(x <= 3.0e38)) return __builtin_inff();
    float f = (float)x;
    if ((double)f < x) f = __uint_as_float(__float_as_uint(f) + 1u);
    return f;
}

// exponent e of the table's power-of-two scale: max|x| * 2^e < 2^15 (0 for an all-zero table)
__device__ __forceinline__ int scale_exp(const unsigned* stats, int word) {
    const float m = __uint_as_float(stats[word]);
    if (!(m > 0.0f) || !(m <= 3.4e38f)) return 0;
    int E;
    frexpf(m, &E);          // m < 2^E
    return 15 - E;
}

// fp16 copy of x * 2^e without subnormals (they are flushed to zero: the residual carries them)
__device__ __forceinline__ _Float16 to_f16(float x, int e) {
    const float y = ldexpf(x, e);
    _Float16 hv = (_Float16)y;
    if (fabsf((float)hv) < 6.103515625e-05f) hv = (_Float16)0.0f;     // 2^-14: the smallest fp16 normal
    return hv;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// max |x| over the finite entries of rows (rows ? rows[r] : r) of a [*][SD] table -> atomicMax on the float bits of stats[word]
// KEYS (the item table, rows == NULL): the pass also leaves a 16-bit norm key per row, the high half of the float bits of its
// sum of squares (fp32, reduced over the 32 consecutive lanes that hold the row; monotone in the norm, about 0.4 % per step).  A
// row whose sum is not finite -- a NaN or an inf entry, or an overflow -- gets the key of +inf.  The key only orders the fp16 pass
// (screen_sortkey_kernel); no bound and no certificate reads it.
constexpr unsigned SCREEN_KEY_NONFINITE = 0x7F80u;
template <bool KEYS>
__global__ __launch_bounds__(256) void screen_maxabs_kernel(const float* __restrict__ tab, const int32_t* __restrict__ rows,
                                                            int64_t n_rows, unsigned* __restrict__ stats, int word,
                                                            uint16_t* __restrict__ keys) {
    const int64_t n4 = n_rows * (SD / 4);
    float m = 0.0f;
    // (n4 and the stride are multiples of 32: the 32 lanes of a row run the same trips)
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n4; e += (int64_t)gridDim.x * 256) {
        const int64_t r = e / (SD / 4);
        const int64_t row = rows ? (int64_t)rows[r] : r;
        const f32x4 x = *reinterpret_cast<const f32x4*>(tab + row * SD + 4 * (e % (SD / 4)));
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float ax = fabsf(x[c]);
            if (ax <= 3.4028235e38f) m = fmaxf(m, ax);     // NaN and inf fail the test: they reach the residuals instead
        }
        if constexpr (KEYS) {
            float ss = x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3];
#pragma unroll
            for (int o = 16; o >= 1; o >>= 1) ss += __shfl_xor(ss, o);
            if ((threadIdx.x & 31) == 0)
                keys[r] = (uint16_t)(ss <= 3.4028235e38f ? __float_as_uint(ss) >> 16 : SCREEN_KEY_NONFINITE);
        }
    }
    __shared__ float red[4];
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float b = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        if (b > 0.0f) atomicMax(stats + word, __float_as_uint(b));
    }
}

// Sums over one row of 16 consecutive lanes (8 elements each): x^2, (x - x^)^2, x^^2 in fp64.
__device__ __forceinline__ void row_sums(const f32x4& x0, const f32x4& x1, _Float16 (&hv)[8], int e, double& sxx, double& sdd,
                                         double& shh) {
    const double inv = ldexp(1.0, -e);
    sxx = 0.0; sdd = 0.0; shh = 0.0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float x = c < 4 ? x0[c & 3] : x1[c & 3];
        hv[c] = to_f16(x, e);
        const double xh = (double)(float)hv[c] * inv;        // exact
        const double dx = (double)x - xh;
        sxx += (double)x * (double)x;
        sdd += dx * dx;
        shh += xh * xh;
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
        sxx += __shfl_xor(sxx, o);
        sdd += __shfl_xor(sdd, o);
        shh += __shfl_xor(shh, o);
    }
}

// B_u (see the head of the file) from the user's three norms and the item maxima, all upper bounds in float: fp64, the absolute
// term of the exact chain's subnormal roundings, and 2^-20 over the roundings of this very sum.  The ONE definition: stage 2's
// predicate and stage 1's margin (screen_users_kernel, screen_margin_kernel) must speak of the same number.
__device__ __forceinline__ double screen_bound(float un, float uhn, float udn, float R, float N, float Nh) {
    const double gd = SD * 0x1p-24 / (1.0 - SD * 0x1p-24), gp = 0x1p-12;
    const double B = (double)un * R + (double)udn * Nh + gd * (double)un * N + gp * (double)uhn * Nh + 0x1p-126;
    return B * (1.0 + 0x1p-20);
}

// an upper bound of sqrt(s) for an fp64 sum of squares (its own rounding error is far below the 2^-30 margin)
__device__ __forceinline__ float up_norm(double s) { return up_float(sqrt(s) * (1.0 + 0x1p-30)); }

// The live-row map of a shard's main range (the global ids [g0, g1), any alignment) under a candidate bitmap: idmap[q] = id of
// the q-th unmasked item, ascending, so the order of the compacted rows is the order of their ids.  Three small kernels, one
// bitmap word per thread: per-block counts, their exclusive scan (one block; it also leaves the total in *n_live), the ids.
constexpr int LIVE_WPB = 256;      // bitmap words per block of the count and id kernels

// unmasked bits of the w-th bitmap word of [g0, g1) (the first and the last word may be partial)
__device__ __forceinline__ unsigned live_word(const uint32_t* __restrict__ bitmap, int64_t w, int64_t g0, int64_t g1) {
    const int64_t w0 = g0 >> 5, n_words = ((g1 - 1) >> 5) - w0 + 1;
    if (w >= n_words) return 0u;
    unsigned m = ~bitmap[w0 + w];
    const int64_t lo = (w0 + w) << 5;
    if (lo < g0) m &= ~0u << (int)(g0 - lo);               // 1 .. 31 bits below the range
    if (lo + 32 > g1) m &= ~0u >> (int)(lo + 32 - g1);     // 1 .. 31 bits above it
    return m;
}

// exclusive sum of v over the block's 256 threads (their order); *total = the block's sum
__device__ __forceinline__ unsigned block_excl_sum(unsigned v, unsigned* total) {
    __shared__ unsigned wsum[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    unsigned before = 0;
    for (int q = 0; q < wv; ++q) before += wsum[q];
    *total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    return before + inc - v;
}

__global__ __launch_bounds__(256) void screen_live_count_kernel(const uint32_t* __restrict__ bitmap, int64_t g0, int64_t g1,
                                                                unsigned* __restrict__ blocksum) {
    const unsigned c = __popc(live_word(bitmap, (int64_t)blockIdx.x * LIVE_WPB + threadIdx.x, g0, g1));
    unsigned total;
    block_excl_sum(c, &total);
    if (threadIdx.x == 0) blocksum[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void screen_live_scan_kernel(unsigned* __restrict__ blocksum, int64_t n_blocks,
                                                               unsigned* __restrict__ n_live) {
    const int64_t per = (n_blocks + 255) / 256;
    const int64_t lo = threadIdx.x * per < n_blocks ? threadIdx.x * per : n_blocks, hi = lo + per < n_blocks ? lo + per : n_blocks;
    unsigned sum = 0;
    for (int64_t q = lo; q < hi; ++q) sum += blocksum[q];
    unsigned total;
    unsigned run = block_excl_sum(sum, &total);
    for (int64_t q = lo; q < hi; ++q) {
        const unsigned c = blocksum[q];
        blocksum[q] = run;
        run += c;
    }
    if (threadIdx.x == 0) *n_live = total;
}

__global__ __launch_bounds__(256) void screen_idmap_kernel(const uint32_t* __restrict__ bitmap, int64_t g0, int64_t g1,
                                                           const unsigned* __restrict__ blocksum, int32_t* __restrict__ idmap) {
    const int64_t w = (int64_t)blockIdx.x * LIVE_WPB + threadIdx.x;
    unsigned m = live_word(bitmap, w, g0, g1);
    unsigned total;
    int64_t pos = (int64_t)blocksum[blockIdx.x] + block_excl_sum(__popc(m), &total);
    const int id0 = (int)(((g0 >> 5) + w) << 5);
    while (m) {
        idmap[pos++] = id0 + __builtin_ctz(m);
        m &= m - 1;
    }
}

// Sort keys of the ordered map: slot q of the ascending map gets the complement of its row's norm key, so that an ascending
// stable sort streams the rows by descending norm, ascending id inside a key; every slot behind the live rows gets the key that
// sorts last (a live all-zero row shares it and stays in front of them: the sort is stable), so the live ids fill [0, n_live).
__global__ __launch_bounds__(256) void screen_sortkey_kernel(const int32_t* __restrict__ idmap, const uint16_t* __restrict__ rowkeys,
                                                             const unsigned* __restrict__ n_live, int64_t item_base, int64_t n_slots,
                                                             uint16_t* __restrict__ skeys) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n_slots) return;
    skeys[q] = q < (int64_t)*n_live ? (uint16_t)~rowkeys[(int64_t)idmap[q] - item_base] : (uint16_t)0xFFFFu;
}

// the norm keys along a sorted map, for crh_score_topk_screen_map
__global__ __launch_bounds__(256) void screen_mapkeys_kernel(const uint16_t* __restrict__ skeys, int64_t n, int32_t* __restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q < n) out[q] = (int32_t)(uint16_t)~skeys[q];
}

// inv[map[q] - g0] = q for the live rows of the map stage 1 streams by (launch_screen_invmap)
__global__ __launch_bounds__(256) void screen_invmap_kernel(const int32_t* __restrict__ map, const unsigned* __restrict__ n_live, int64_t g0,
                                                            int32_t* __restrict__ inv) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q < (int64_t)*n_live) inv[(int64_t)map[q] - g0] = (int32_t)q;
}

// The rated-tile flags (ScoreArgs::rated_tiles), one thread per rated entry of the call (grid-stride: the host does not know their
// number).  The entry's owner is the last slot whose list starts at or before it; an id outside the main range [g0, g1), or cold
// under the bitmap, is not in the stream and sets nothing.  nb = 256-byte pieces per workgroup.
__global__ __launch_bounds__(256) void screen_rated_tiles_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                 int64_t n_users, const uint32_t* __restrict__ bitmap, int64_t g0, int64_t g1,
                                                                 const int32_t* __restrict__ inv, uint32_t* __restrict__ flags, int64_t nb) {
    const int64_t e0 = rowptr[0], e1 = rowptr[n_users];
    for (int64_t e = e0 + (int64_t)blockIdx.x * 256 + threadIdx.x; e < e1; e += (int64_t)gridDim.x * 256) {
        const int64_t v = col[e];
        if (v < g0 || v >= g1) continue;
        if ((bitmap[v >> 5] >> (v & 31)) & 1u) continue;
        int64_t lo = 0, hi = n_users;                 // the owner: the last slot with rowptr[slot] <= e
        while (hi - lo > 1) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (rowptr[mid] <= e) lo = mid;
            else hi = mid;
        }
        const int64_t wave = lo >> 7, t = (int64_t)inv[v - g0] >> 5;
        atomicOr(flags + ((wave >> 2) * nb * 64 + (t >> 3)), 1u << (4 * (int)(t & 7) + (int)(wave & 3)));
    }
}

// Item shard -> fp16 in the fragment-ordered packed layout of pack_items_f16_kernel<128> (tile t, unit c = 8 elements of row r at
// ((t * 8 + c / 2) * 64 + (c & 1) * 32 + r)), bitmap-masked rows zero; the maxima of |v - v^|, |v|, |v^| over the unmasked rows
// go to stats[2..4].  Grid-stride over tiles; 16 lanes per row.
// idmap != NULL (the compacted copy): the first `prefix` rows (a multiple of 32) as above; behind them destination row q is the
// q-th unmasked item of the main range, shard row idmap[q] - item_base -- still one contiguous 512-byte read per row.  The masked
// rows are neither read nor written, the rows behind the last live one in its tile are zeros (nobody selects them), and the
// maxima cover exactly the rows they cover without the compaction.
__global__ __launch_bounds__(256) void screen_items_kernel(const float* __restrict__ v, int64_t n_items, const uint32_t* __restrict__ bitmap,
                                                           int64_t item_base, _Float16* __restrict__ packed, unsigned* __restrict__ stats,
                                                           int64_t prefix, const int32_t* __restrict__ idmap) {
    const int e = scale_exp(stats, 0);
    const int64_t TP = prefix >> 5, n_live = idmap ? (int64_t)stats[SCREEN_STAT_LIVE] : 0;
    const int64_t T = idmap ? TP + ((n_live + 31) >> 5) : (n_items + 31) >> 5;
    float mr = 0.0f, mn = 0.0f, mh = 0.0f;
    u32x4* dst = reinterpret_cast<u32x4*>(packed);
    for (int64_t t = blockIdx.x; t < T; t += gridDim.x) {
        for (int p = 0; p < 2; ++p) {
            const int u = threadIdx.x + 256 * p, r = u >> 4, c = u & 15;
            int64_t row = (t << 5) + r;
            bool masked;
            if (idmap != nullptr && t >= TP) {
                const int64_t q = row - prefix;
                masked = q >= n_live;                     // (n_live >= 1 here)
                row = (int64_t)idmap[masked ? n_live - 1 : q] - item_base;
            } else {
                if (row >= n_items) row = n_items - 1;        // the tail tile repeats the last row (as the pack kernels do)
                masked = bitmap != nullptr && ((bitmap[(item_base + row) >> 5] >> ((item_base + row) & 31)) & 1u);
            }
            const float* src = v + row * SD + 8 * c;
            const f32x4 x0 = *reinterpret_cast<const f32x4*>(src), x1 = *reinterpret_cast<const f32x4*>(src + 4);
            _Float16 hv[8];
            double sxx, sdd, shh;
            row_sums(x0, x1, hv, e, sxx, sdd, shh);
            u32x4 o = u32x4{0u, 0u, 0u, 0u};
            if (!masked) {
                o = __builtin_bit_cast(u32x4, f16x8{hv[0], hv[1], hv[2], hv[3], hv[4], hv[5], hv[6], hv[7]});
                mr = fmaxf(mr, up_norm(sdd));
                mn = fmaxf(mn, up_norm(sxx));
                mh = fmaxf(mh, up_norm(shh));
                if (sdd != sdd || sxx != sxx) mr = __builtin_inff();     // NaN input: fmaxf would drop it
            }
            dst[(t * 8 + (c >> 1)) * 64 + (c & 1) * 32 + r] = o;
        }
    }
    __shared__ float red[3][4];
    mr = wave_max(mr);
    mn = wave_max(mn);
    mh = wave_max(mh);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = mr;
        red[1][threadIdx.x >> 6] = mn;
        red[2][threadIdx.x >> 6] = mh;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const float b = fmaxf(fmaxf(red[threadIdx.x][0], red[threadIdx.x][1]), fmaxf(red[threadIdx.x][2], red[threadIdx.x][3]));
        if (b > 0.0f) atomicMax(stats + 2 + threadIdx.x, __float_as_uint(b));
    }
}

// User block (in `users` order) -> fp16 row-major [n_users][128]; per user |u|, |u^|, |u - u^| (upper bounds) into ustat[3 j ..].
// The item maxima are in the stats block by now (built in front of this kernel, or copied from the prepared state): the largest B_u of
// the call goes to stats[SCREEN_STAT_MAXB] (float bits, atomicMax as R, N, N^; a non-finite B_u -- a non-finite row makes a norm
// +inf -- goes in as +inf), for the margin of stage 1 (screen_margin_kernel).
__global__ __launch_bounds__(256) void screen_users_kernel(const float* __restrict__ uemb, const int32_t* __restrict__ users,
                                                           int64_t n_users, _Float16* __restrict__ uh, float* __restrict__ ustat,
                                                           unsigned* __restrict__ stats) {
    const int e = scale_exp(stats, 1);
    const float R = __uint_as_float(stats[2]), N = __uint_as_float(stats[3]), Nh = __uint_as_float(stats[4]);
    float mb = 0.0f;
    const int64_t n_units = n_users * 16;
    for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < ((n_units + 255) & ~(int64_t)255); w += (int64_t)gridDim.x * 256) {
        const int64_t j = (w < n_units ? w : n_units - 1) >> 4;      // (the shuffles need every lane of the row group)
        const int c = (int)(w & 15);
        const int64_t row = users ? (int64_t)users[j] : j;
        const float* src = uemb + row * SD + 8 * c;
        const f32x4 x0 = *reinterpret_cast<const f32x4*>(src), x1 = *reinterpret_cast<const f32x4*>(src + 4);
        _Float16 hv[8];
        double sxx, sdd, shh;
        row_sums(x0, x1, hv, e, sxx, sdd, shh);
        if (w < n_units) {
            reinterpret_cast<u32x4*>(uh)[j * 16 + c] = __builtin_bit_cast(u32x4, f16x8{hv[0], hv[1], hv[2], hv[3], hv[4], hv[5], hv[6], hv[7]});
            if (c == 0) {
                const bool bad = sxx != sxx || sdd != sdd;
                const float un = bad ? __builtin_inff() : up_norm(sxx), uhn = bad ? __builtin_inff() : up_norm(shh);
                const float udn = bad ? __builtin_inff() : up_norm(sdd);
                ustat[3 * j + 0] = un;
                ustat[3 * j + 1] = uhn;
                ustat[3 * j + 2] = udn;
                // (from the floats stage 2 reads; up_float turns NaN and overflow into +inf)
                mb = fmaxf(mb, up_float(screen_bound(un, uhn, udn, R, N, Nh)));
            }
        }
    }
    __shared__ float red[4];
    mb = wave_max(mb);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mb;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float b = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        if (b > 0.0f) atomicMax(stats + SCREEN_STAT_MAXB, __float_as_uint(b));
    }
}

// The margin of stage 1's thresholds, one thread: M = 2 (1 + 2^-10) max B_u in the fp16 kernel's score units (the
// two table scales are powers of two: exact), rounded UP to a float and never below the smallest normal one -- so M > 2 B_u for every
// user of the call after every rounding, and the 2^-10 covers the kernel's float subtraction L[k-1] - M (B_u >= 2^-12 |a| for every
// approximate score a of the user).  A non-finite bound, or margin_on == 0, gives +inf: the rule is off for the call.
__global__ void screen_margin_kernel(unsigned* __restrict__ stats, int margin_on) {
    const float maxb = __uint_as_float(stats[SCREEN_STAT_MAXB]);
    float M = __builtin_inff();
    if (margin_on && maxb <= 3.4028235e38f) {             // (NaN fails)
        const double m = 2.0 * (1.0 + 0x1p-10) * (double)maxb * ldexp(1.0, scale_exp(stats, 0) + scale_exp(stats, 1));
        M = fmaxf(up_float(m), 0x1p-126f);
    }
    stats[SCREEN_STAT_MARGIN] = __float_as_uint(M);
}

// the canonical score: fmaf chain over k ascending from +0 (oracle/topk_oracle.c)
__device__ __forceinline__ float exact_chain(const float* __restrict__ u, const float* __restrict__ v) {
    float s = 0.0f;
#pragma unroll 8
    for (int q = 0; q < SD; q += 4) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(u + q), b = *reinterpret_cast<const f32x4*>(v + q);
        s = __builtin_fmaf(a.x, b.x, s);
        s = __builtin_fmaf(a.y, b.y, s);
        s = __builtin_fmaf(a.z, b.z, s);
        s = __builtin_fmaf(a.w, b.w, s);
    }
    return s;
}

// is gi in the ascending list col[lo, hi)?  (one lane, binary search)
__device__ __forceinline__ bool lane_in_list(const int32_t* __restrict__ col, int64_t lo, int64_t hi, int gi) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const int x = col[mid];
        if (x == gi) return true;
        if (x < gi) lo = mid + 1;
        else hi = mid;
    }
    return false;
}

// Stage 2: one wave per user, one lane per candidate.  A certified user's k best candidates by (exact score desc, id asc) are its
// answer; every other user is appended to fail_list (count in stats[5]).
__global__ __launch_bounds__(256) void screen_certify_kernel(ScreenArgs s) {
    const int lane = threadIdx.x & 63;
    const int64_t slot = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slot >= s.n_users) return;                       // wave-uniform
    const int KP = s.kp, K = s.k;
    const bool mine = lane < KP;
    int gi = CRH_PAD_IDX;
    float a = CRH_NEG_INF;
    if (mine) {
        gi = s.cand_idx[slot * KP + lane];
        a = s.cand_score[slot * KP + lane];
    }
    const bool real = mine && gi != CRH_PAD_IDX && (int64_t)gi >= s.item_base && (int64_t)gi < s.item_base + s.n_items;
    bool masked = false;
    if (real && s.bitmap) masked = (s.bitmap[gi >> 5] >> (gi & 31)) & 1u;
    if (real && !masked && s.rated_rowptr) masked = lane_in_list(s.rated_col, s.rated_rowptr[slot], s.rated_rowptr[slot + 1], gi);
    const int64_t urow = s.users ? (int64_t)s.users[slot] : slot;
    float sc = CRH_NEG_INF;
    if (real) sc = exact_chain(s.user_emb + urow * SD, s.item_emb + ((int64_t)gi - s.item_base) * SD);
    const bool ok = !mine || (real && !masked && __builtin_isfinite(a) && __builtin_isfinite(sc));
    // rank of this lane's candidate among the KP by the canonical key (ids are distinct)
    int rank = 0;
    for (int j = 0; j < KP; ++j) {
        const float sj = __shfl(sc, j);
        const int ij = __shfl(gi, j);
        rank += (j != lane && crh_better(sj, ij, sc, gi)) ? 1 : 0;
    }
    const unsigned long long kth = __ballot(mine && rank == K - 1);
    const float ek = __shfl(sc, kth ? __builtin_ctzll(kth) : 0);
    const float a_last = __shfl(a, KP - 1);
    const float a_k = __shfl(a, K - 1);
    bool cert = s.mode != 3 && __ballot(!ok) == 0ull && kth != 0ull;
    if (cert) {
        const float* us = s.ustat + 3 * slot;
        const float R = __uint_as_float(s.stats[2]), N = __uint_as_float(s.stats[3]), Nh = __uint_as_float(s.stats[4]);
        const double B = screen_bound(us[0], us[1], us[2], R, N, Nh);
        const double unscale = ldexp(1.0, -(scale_exp(s.stats, 0) + scale_exp(s.stats, 1)));
        const double A = (double)a_last * unscale;         // exact
        double thr = A + B;
        thr += fabs(thr) * 0x1p-50;                        // the rounding of that sum, upward
        cert = (double)ek > thr && ek > CRH_MASKED_SCORE;  // NaN anywhere fails both
        // stage 1's margin rule kept out of the list only rows below a_k - M: what it dropped lies below (a_k - M) + B_u.  With
        // M > 2 B_u this holds whenever the bound does (e_k >= a_k - B_u), so it moves no count; M = +inf (the rule off) passes
        const float Mk = __uint_as_float(s.stats[SCREEN_STAT_MARGIN]);
        if (Mk <= 3.4028235e38f) {
            double thr_m = ((double)a_k - (double)Mk) * unscale + B;
            thr_m += fabs(thr_m) * 0x1p-50;
            cert = cert && (double)ek > thr_m;
        }
    }
    if (cert) {
        if (mine && rank < K) {
            s.out_score[slot * K + rank] = sc;
            s.out_idx[slot * K + rank] = gi;
        }
    } else if (lane == 0) {
        const unsigned f = atomicAdd(s.stats + 5, 1u);
        s.fail_list[f] = (int32_t)slot;
    }
}

// Item slices per uncertified user in the fallback, from the count (read on the device by every stage-3 kernel, so they all agree):
// enough (user x slice) work items to fill one resident round of the chip (FB_WAVES), at least FB_MIN_ITEMS items per slice, at most
// FB_SLICES_MAX (two merge levels of FB_FANIN), and never more lists than the scratch holds (s.n_slices per user of the call: since
// count <= n_users, that leaves at least s.n_slices each).  One uncertified user of the headline: 4 096 slices of 2 441 items
// instead of 64 of 156 250 -- the fallback was a handful of latency-bound waves walking the table.
constexpr int64_t FB_WAVES = 2048 * 4;   // the fallback's grid: 2 048 workgroups of four waves
constexpr int64_t FB_MIN_ITEMS = 1024;
constexpr int FB_FANIN = 64;             // lists merged by one wave per merge level
constexpr int FB_SLICES_MAX = FB_FANIN * FB_FANIN;
__device__ __forceinline__ int fb_slices(const ScreenArgs& s, int64_t count) {
    if (count <= 0) return 1;
    int64_t S = (FB_WAVES + count - 1) / count;
    const int64_t by_items = (s.n_items + FB_MIN_ITEMS - 1) / FB_MIN_ITEMS;
    const int64_t by_scratch = s.n_users * s.n_slices / count;
    if (S > by_items) S = by_items;
    if (S > by_scratch) S = by_scratch;
    if (S > FB_SLICES_MAX) S = FB_SLICES_MAX;
    return S < 1 ? 1 : (int)S;
}

// Stage 3a: exact per-(uncertified user, item slice) lists, grid-stride over count x fb_slices work items (the count is read
// here, on the device).  Semantics of the fused selection's slow path: an item is a candidate when its raw score (a bitmap-masked
// item scores against a zero row, as in the packed copies) is above the list's threshold; masked candidates enter at -1e9.
__global__ __launch_bounds__(256) void screen_fallback_kernel(ScreenArgs s) {
    __shared__ float ush[4][SD];
    __shared__ float lsh[4][32];
    __shared__ int lih[4][32];
    __shared__ int cnth[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int K = s.k;
    const int64_t count = s.stats[5];
    const int S = fb_slices(s, count);
    const int64_t n_work = count * S;
    float* ls = lsh[wv];
    int* li = lih[wv];
    int* cnt = &cnth[wv];
    for (int64_t w = (int64_t)blockIdx.x * 4 + wv; w < n_work; w += (int64_t)gridDim.x * 4) {
        const int64_t f = w / S;
        const int z = (int)(w % S);
        const int64_t slot = s.fail_list[f];
        const int64_t urow = s.users ? (int64_t)s.users[slot] : slot;
        ush[wv][lane] = s.user_emb[urow * SD + lane];
        ush[wv][lane + 64] = s.user_emb[urow * SD + lane + 64];
        if (lane == 0) *cnt = 0;
        const int64_t lo = s.n_items * z / S, hi = s.n_items * (z + 1) / S;
        float tau = CRH_NEG_INF;
        for (int64_t base = lo; base < hi; base += 64) {
            const int64_t i = base + lane;
            const bool valid = i < hi;
            const int gl = (int)(s.item_base + (valid ? i : lo));
            const bool bm = valid && s.bitmap && ((s.bitmap[gl >> 5] >> (gl & 31)) & 1u);
            float raw = CRH_NEG_INF;
            if (valid) {
                if (bm) {
                    raw = 0.0f;
#pragma unroll 8
                    for (int q = 0; q < SD; ++q) raw = __builtin_fmaf(ush[wv][q], 0.0f, raw);
                } else {
                    raw = exact_chain(ush[wv], s.item_emb + i * SD);
                }
            }
            unsigned long long cand = __ballot(valid && raw > tau);
            const unsigned long long bms = __ballot(bm);
            while (cand) {
                const int L = __builtin_ctzll(cand);
                cand &= cand - 1;
                float sc = __shfl(raw, L);
                const int g = (int)(s.item_base + base + L);
                const int n = __builtin_amdgcn_readfirstlane(*cnt);
                if (wave_list_rejects(ls, li, n, K, sc, g)) continue;
                bool masked = (bms >> L) & 1ull;
                if (!masked && s.rated_rowptr) masked = wave_is_masked(g, slot, s.rated_rowptr, s.rated_col, nullptr, lane);
                if (masked) sc = CRH_MASKED_SCORE;
                wave_list_insert(ls, li, cnt, K, sc, g, lane);
                tau = wave_list_tau(ls, __builtin_amdgcn_readfirstlane(*cnt), K);
            }
        }
        const int n = __builtin_amdgcn_readfirstlane(*cnt);
        const int64_t o = (f * S + z) * K;
        wave_list_store(ls, li, n, K, s.part_score + o, s.part_idx + o, lane);
    }
}

// Stage 3b: canonical merge of an uncertified user's slice lists, FB_FANIN lists per wave and level.  Level 0 merges slices
// [64 g, 64 g + 64) into the list of slice 64 g; level 1 merges those (slices 0, 64, 128, ...) into the output row.  Whichever
// level sees every slice of a user in one group (level 0 when fb_slices <= 64) writes the output row; a later level has nothing
// left to do.  A group's first list is read before its merged list overwrites it, by the same wave: merging in place is safe.
__global__ __launch_bounds__(256) void screen_fallback_merge_kernel(ScreenArgs s, int level) {
    __shared__ float lsh[4][32];
    __shared__ int lih[4][32];
    __shared__ int cnth[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int K = s.k;
    const int64_t count = s.stats[5];
    const int S = fb_slices(s, count);
    const int last = S <= FB_FANIN ? 0 : 1;
    if (level > last) return;                              // uniform over the grid
    const int stride = level == 0 ? 1 : FB_FANIN;          // slice distance of the lists merged at this level
    const int span = stride * FB_FANIN;                     // slices covered by one group
    const int G = (S + span - 1) / span;                    // groups per user
    float* ls = lsh[wv];
    int* li = lih[wv];
    int* cnt = &cnth[wv];
    for (int64_t w = (int64_t)blockIdx.x * 4 + wv; w < count * G; w += (int64_t)gridDim.x * 4) {
        const int64_t f = w / G;
        const int z0 = (int)(w % G) * span;
        if (lane == 0) *cnt = 0;
        for (int z = z0; z < z0 + span && z < S; z += stride) {
            const int64_t o = (f * S + z) * K;
            const float es = lane < K ? s.part_score[o + lane] : CRH_NEG_INF;
            const int ei = lane < K ? s.part_idx[o + lane] : CRH_PAD_IDX;
            unsigned long long m = __ballot(lane < K && ei != CRH_PAD_IDX);
            while (m) {
                const int L = __builtin_ctzll(m);
                m &= m - 1;
                const float sc = __shfl(es, L);
                const int g = __shfl(ei, L);
                const int n = __builtin_amdgcn_readfirstlane(*cnt);
                if (n >= K && !crh_better(sc, g, ls[K - 1], li[K - 1])) break;   // the slice list is sorted: the rest cannot enter
                wave_list_insert(ls, li, cnt, K, sc, g, lane);
            }
        }
        const int n = __builtin_amdgcn_readfirstlane(*cnt);
        if (level == last) {
            const int64_t slot = s.fail_list[f];
            wave_list_store(ls, li, n, K, s.out_score + slot * K, s.out_idx + slot * K, lane);
        } else {
            const int64_t o = (f * S + z0) * K;
            wave_list_store(ls, li, n, K, s.part_score + o, s.part_idx + o, lane);
        }
    }
}

}  // namespace

// slice lists per user the workspace holds for the fallback (screen_layout; the kernels pick their own count inside it)
int screen_fallback_slices(int64_t n_items) {
    const int64_t s = n_items / 4096;
    return (int)(s < 1 ? 1 : (s > FB_SCRATCH_SLICES ? FB_SCRATCH_SLICES : s));
}

// block sums of the live-row scan (screen_live_*_kernel): one word per LIVE_WPB bitmap words of the main range
size_t screen_scan_bytes(int64_t n_main) { return (size_t)((n_main + 31) / 32 / LIVE_WPB + 2) * sizeof(unsigned); }

// slots of the live-row map of a main range of n_main items: whole tiles plus the one the id DMA of the last tile may touch
int64_t screen_map_slots(int64_t n_main) { return ((n_main + 31) / 32 + 1) * 32; }

// Temporary storage reserved for the ordered map's sort of n_slots (16-bit key, id) pairs.  The radix sort asks for its
// alternate key and id buffers (6 bytes per pair), digit histograms and one look-back word per digit and block (below 2 bytes per
// pair at any block size it is built with); what it asks for is checked against this when it runs (launch_screen_map).
size_t screen_sort_bytes(int64_t n_slots) { return (size_t)n_slots * 8 + ((size_t)1 << 20); }

// The live-row map of [item_base + prefix, item_base + n_items): ascending in idmap; with ord also sorted stably by descending
// norm key into ord->idmap (the keys along it in ord->skeys_out).  No host synchronisation: the sort covers every slot.
int launch_screen_map(const uint32_t* bitmap, int64_t item_base, int64_t n_items, int64_t prefix, unsigned* n_live, unsigned* scan,
                      int32_t* idmap, const ScreenOrder* ord, hipStream_t st) {
    const int64_t g0 = item_base + prefix, g1 = item_base + n_items;
    const int64_t n_words = ((g1 - 1) >> 5) - (g0 >> 5) + 1, nb = (n_words + LIVE_WPB - 1) / LIVE_WPB;
    hipLaunchKernelGGL(screen_live_count_kernel, dim3((unsigned)nb), dim3(256), 0, st, bitmap, g0, g1, scan);
    CRH_HIP(hipGetLastError());
    hipLaunchKernelGGL(screen_live_scan_kernel, dim3(1), dim3(256), 0, st, scan, nb, n_live);
    CRH_HIP(hipGetLastError());
    hipLaunchKernelGGL(screen_idmap_kernel, dim3((unsigned)nb), dim3(256), 0, st, bitmap, g0, g1, scan, idmap);
    CRH_HIP(hipGetLastError());
    if (ord == nullptr) return CRH_OK;
    const int64_t n_slots = screen_map_slots(n_items - prefix);
    hipLaunchKernelGGL(screen_sortkey_kernel, dim3((unsigned)((n_slots + 255) / 256)), dim3(256), 0, st, idmap, ord->rowkeys, n_live,
                       item_base, n_slots, ord->skeys_in);
    CRH_HIP(hipGetLastError());
    size_t need = 0;
    CRH_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, need, ord->skeys_in, ord->skeys_out, idmap, ord->idmap, (int)n_slots, 0, 16, st));
    if (need > ord->sort_tmp_bytes) {
        crh_set_error("screened route: the ordered map's sort asks for %zu bytes of temporary storage, %zu are reserved", need,
                      ord->sort_tmp_bytes);
        return CRH_ERR_WS;
    }
    need = ord->sort_tmp_bytes;
    CRH_HIP(hipcub::DeviceRadixSort::SortPairs(ord->sort_tmp, need, ord->skeys_in, ord->skeys_out, idmap, ord->idmap, (int)n_slots, 0, 16, st));
    return CRH_OK;
}

int launch_screen_invmap(const int32_t* map, const unsigned* n_live, int64_t g0, int64_t n_main, int32_t* inv, hipStream_t st) {
    hipLaunchKernelGGL(screen_invmap_kernel, dim3((unsigned)((n_main + 255) / 256)), dim3(256), 0, st, map, n_live, g0, inv);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

size_t screen_rated_tiles_bytes(int64_t n_users, int64_t n_main) {
    const int64_t groups = ((n_users + 127) / 128 + 3) / 4;
    return (size_t)(groups * screen_rated_blocks(n_main)) * 256;
}

int launch_screen_rated_tiles(const int64_t* rated_rowptr, const int32_t* rated_col, int64_t n_users, const uint32_t* bitmap, int64_t g0,
                              int64_t g1, const int32_t* inv, uint32_t* flags, hipStream_t st) {
    CRH_HIP(hipMemsetAsync(flags, 0, screen_rated_tiles_bytes(n_users, g1 - g0), st));
    hipLaunchKernelGGL(screen_rated_tiles_kernel, dim3(4096), dim3(256), 0, st, rated_rowptr, rated_col, n_users, bitmap, g0, g1, inv, flags,
                       screen_rated_blocks(g1 - g0));
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

int launch_screen_prep_items(const ScreenArgs& s, unsigned* stats, _Float16* packed, int64_t prefix, int32_t* idmap, unsigned* scan,
                             const ScreenOrder* ord, hipStream_t st) {
    const int64_t T = (s.n_items + 31) / 32;     // (compacted: the upper bound; the kernel walks the live tiles)
    if (ord != nullptr)
        hipLaunchKernelGGL(screen_maxabs_kernel<true>, dim3(2048), dim3(256), 0, st, s.item_emb, nullptr, s.n_items, stats, 0, ord->rowkeys);
    else
        hipLaunchKernelGGL(screen_maxabs_kernel<false>, dim3(2048), dim3(256), 0, st, s.item_emb, nullptr, s.n_items, stats, 0, nullptr);
    CRH_HIP(hipGetLastError());
    if (idmap != nullptr) {
        const int rc = launch_screen_map(s.bitmap, s.item_base, s.n_items, prefix, stats + SCREEN_STAT_LIVE, scan, idmap, ord, st);
        if (rc != CRH_OK) return rc;
        if (ord != nullptr) idmap = ord->idmap;
    }
    hipLaunchKernelGGL(screen_items_kernel, dim3((unsigned)(T < 4096 ? T : 4096)), dim3(256), 0, st, s.item_emb, s.n_items, s.bitmap,
                       s.item_base, packed, stats, prefix, idmap);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

int launch_screen_prep_users(const ScreenArgs& s, _Float16* uh, int margin_on, hipStream_t st) {
    hipLaunchKernelGGL(screen_maxabs_kernel<false>, dim3(256), dim3(256), 0, st, s.user_emb, s.users, s.n_users, s.stats, 1, nullptr);
    CRH_HIP(hipGetLastError());
    const int64_t ub = (s.n_users * 16 + 255) / 256;
    hipLaunchKernelGGL(screen_users_kernel, dim3((unsigned)(ub < 2048 ? ub : 2048)), dim3(256), 0, st, s.user_emb, s.users, s.n_users,
                       uh, s.ustat, s.stats);
    CRH_HIP(hipGetLastError());
    hipLaunchKernelGGL(screen_margin_kernel, dim3(1), dim3(1), 0, st, s.stats, margin_on);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

// Only the map construction of stage 0, into buffers of its own (crh_score_topk_screen_map; synchronises): map_out and keys_out take
// n_items - prefix entries each, the first *count of them meaningful.
int screen_map_only(const uint32_t* bitmap, const float* item_emb, int64_t n_items, int64_t item_base, int64_t prefix, int ordered,
                    int32_t* map_out, int32_t* keys_out, int64_t* count, hipStream_t st, const int64_t* rated_rowptr,
                    const int32_t* rated_col, int64_t n_users, uint32_t* flags_out) {
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const int64_t n_main = n_items - prefix, n_slots = screen_map_slots(n_main);
    const size_t o_scan = 256, o_map = o_scan + al(screen_scan_bytes(n_main)), o_rk = o_map + al((size_t)n_slots * 4),
                 o_k0 = o_rk + al((size_t)n_items * 2), o_k1 = o_k0 + al((size_t)n_slots * 2), o_m1 = o_k1 + al((size_t)n_slots * 2),
                 o_tmp = o_m1 + al((size_t)n_slots * 4), o_inv = o_tmp + al(screen_sort_bytes(n_slots)),
                 total = o_inv + (flags_out ? al((size_t)n_main * 4) : 0);
    char* buf = nullptr;
    CRH_HIP(hipMalloc(reinterpret_cast<void**>(&buf), total));
    ScreenOrder ord;
    ord.rowkeys = reinterpret_cast<uint16_t*>(buf + o_rk);
    ord.skeys_in = reinterpret_cast<uint16_t*>(buf + o_k0);
    ord.skeys_out = reinterpret_cast<uint16_t*>(buf + o_k1);
    ord.idmap = reinterpret_cast<int32_t*>(buf + o_m1);
    ord.sort_tmp = buf + o_tmp;
    ord.sort_tmp_bytes = screen_sort_bytes(n_slots);
    unsigned* stats = reinterpret_cast<unsigned*>(buf);
    int32_t* idmap = reinterpret_cast<int32_t*>(buf + o_map);
    int rc = CRH_OK;
    unsigned live = 0;
    hipError_t e = hipMemsetAsync(buf, 0, 256, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(screen_maxabs_kernel<true>, dim3(2048), dim3(256), 0, st, item_emb, nullptr, n_items, stats, 0, ord.rowkeys);
        e = hipGetLastError();
    }
    if (e == hipSuccess) rc = launch_screen_map(bitmap, item_base, n_items, prefix, stats + SCREEN_STAT_LIVE, reinterpret_cast<unsigned*>(buf + o_scan), idmap, &ord, st);
    if (e == hipSuccess && rc == CRH_OK) {
        // (the unordered map's keys: those of its rows, as the sort received them)
        hipLaunchKernelGGL(screen_mapkeys_kernel, dim3((unsigned)((n_main + 255) / 256)), dim3(256), 0, st,
                           ordered ? ord.skeys_out : ord.skeys_in, n_main, keys_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess && rc == CRH_OK)
        e = hipMemcpyAsync(map_out, ordered ? ord.idmap : idmap, (size_t)n_main * 4, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && rc == CRH_OK && flags_out != nullptr) {
        int32_t* inv = reinterpret_cast<int32_t*>(buf + o_inv);
        rc = launch_screen_invmap(ordered ? ord.idmap : idmap, stats + SCREEN_STAT_LIVE, item_base + prefix, n_main, inv, st);
        if (rc == CRH_OK)
            rc = launch_screen_rated_tiles(rated_rowptr, rated_col, n_users, bitmap, item_base + prefix, item_base + n_items, inv, flags_out, st);
    }
    if (e == hipSuccess && rc == CRH_OK) e = hipMemcpyAsync(&live, stats + SCREEN_STAT_LIVE, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(buf);
    CRH_HIP(e);
    if (rc == CRH_OK) *count = (int64_t)live;
    return rc;
}

int launch_screen_certify(const ScreenArgs& s, hipStream_t st) {
    hipLaunchKernelGGL(screen_certify_kernel, dim3((unsigned)((s.n_users + 3) / 4)), dim3(256), 0, st, s);
    CRH_HIP(hipGetLastError());
    // the fallback's grid does not depend on the count (it is on the device): one resident round of the chip (fb_slices)
    hipLaunchKernelGGL(screen_fallback_kernel, dim3((unsigned)(FB_WAVES / 4)), dim3(256), 0, st, s);
    CRH_HIP(hipGetLastError());
    for (int level = 0; level < 2; ++level) {
        hipLaunchKernelGGL(screen_fallback_merge_kernel, dim3(512), dim3(256), 0, st, s, level);
        CRH_HIP(hipGetLastError());
    }
    return CRH_OK;
}

}  // namespace crh_score
