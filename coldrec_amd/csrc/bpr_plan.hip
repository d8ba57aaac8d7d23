// Builders of the BPR batch plan (layout: bpr_plan.h) for gfx950.
//
// What is in this file:
//   * the LDS builder: one workgroup per side of a batch sorts the batch's (row | entry) keys in LDS (bitonic) and emits
//     the reverse index; a second launch writes header and heavy list (crh_bpr_plan_build, batches up to 8 192 triples);
//   * the large builder: chunk sorts in LDS, merge-path passes in global memory, a two-pass emit, and the two-pass heavy
//     lists (crh_bpr_plan_build_large, batches up to 524 288);
//   * the host builder (crh_bpr_plan_build_host), crh_bpr_plan_ints and crh_bpr_heavy_threshold.
// All three builders write the same ints for the same batch.
#include <algorithm>
#include <vector>

#include "bpr_plan.h"

namespace {

// ---------------------------------------------------------------- plan builder (device)
// One workgroup per batch side sorts the side's (row | entry) keys in LDS (bitonic; see PlanKey for the two widths) and
// emits the reverse index in the layout bpr_bwd_rows_kernel reads.  An epoch of S-ML (159 batches of
// 4096 triples) is one launch of 2 x 159 workgroups.
constexpr int PLAN_THREADS = 1024;

// Sort key of a plan entry: row id above the payload (entry index in the batch, role bit for the item side).
// 64 bits in general; 32 bits when every row id of the batch is below 2^17 (MovieLens / CiteULike scale: half the
// LDS traffic of the sort, 32-bit compares): row << 14 | role << 13 | entry, entry < 8192.
template <typename K>
struct PlanKey;
template <>
struct PlanKey<unsigned long long> {
    static constexpr unsigned long long INVALID = ~0ull;
    __device__ static unsigned long long make(uint32_t row, unsigned e, unsigned role) {
        return ((unsigned long long)row << 31) | e | (role << 30);
    }
    __device__ static int32_t row(unsigned long long k) { return (int32_t)(k >> 31); }
    __device__ static int32_t entry(unsigned long long k) { return (int32_t)(k & 0x7fffffffull); }   // e | role << 30
};
template <>
struct PlanKey<uint32_t> {
    static constexpr uint32_t INVALID = ~0u;
    __device__ static uint32_t make(uint32_t row, unsigned e, unsigned role) { return (row << 14) | (role << 13) | e; }
    __device__ static int32_t row(uint32_t k) { return (int32_t)(k >> 14); }
    __device__ static int32_t entry(uint32_t k) { return (int32_t)((k & 0x1fffu) | (((k >> 13) & 1u) << 30)); }
};

// LDS index of key i: eight keys of padding after every 64.  A pass whose eight keys per thread are 8 apart (threads
// t, t+8, .. of a wave then sit 64 keys apart) would put eight lanes on every bank; with the padding the 64 lanes of a
// read fall on 64 different banks for every stride the sort uses (1, 8, 64, 512, 4096), and a thread's eight
// consecutive keys stay contiguous and 32-B aligned.
__device__ __forceinline__ int plan_pk(int i) { return i + ((i >> 6) << 3); }
__host__ __device__ constexpr size_t plan_padded_keys(size_t n) { return n + ((n + 63) / 64) * 8; }

// Bitonic sort of P keys (a power of two) in LDS by one workgroup, ascending.  Written without direction bits: the
// first sub-stage of stage k compares key i with key i ^ (k - 1) (the mirrored position in its block of k), the others i
// with i ^ stride, and every compare puts the smaller key at the lower index -- two instructions (min, max) per
// compare-exchange of 32-bit keys.  A thread takes the 2^NB keys whose indices differ in NB consecutive bit positions,
// runs those NB sub-stages on them in registers and writes them back: a stage of log2(k) sub-stages costs
// ceil(log2(k) / 3) passes over LDS (one barrier each) instead of log2(k), and the stages k = 2, 4, 8 are one pass.
// P = 8192: 33 passes instead of 91.
template <typename K>
__device__ __forceinline__ void bitonic_cx(K& x, K& y) {
    const bool sw = y < x;
    const K lo = sw ? y : x, hi = sw ? x : y;
    x = lo;
    y = hi;
}
template <>
__device__ __forceinline__ void bitonic_cx<uint32_t>(uint32_t& x, uint32_t& y) {
    const uint32_t lo = min(x, y), hi = max(x, y);
    x = lo;
    y = hi;
}

// Sub-stages with strides 2^b, 2^(b-1) .. 2^(b-NB+1).  FIRST: 2^b is the first sub-stage of its stage (k = 2^(b+1)):
// the upper half of a thread's keys then comes from the mirrored low bits, so that register c pairs with register ~c.
template <typename K, int NB, bool FIRST>
__device__ __forceinline__ void bitonic_pass(K* keys, int P, int b) {
    constexpr int N = 1 << NB;
    const int lowbit = b - NB + 1;
    const int lowmask = (1 << lowbit) - 1;
    for (int t = threadIdx.x; t < (P >> NB); t += PLAN_THREADS) {
        const int hi = (t >> lowbit) << (b + 1), lo = t & lowmask;
        const int lo_up = FIRST ? lowmask - lo : lo;
        K v[N];
#pragma unroll
        for (int c = 0; c < N; ++c) v[c] = keys[plan_pk(hi | (c << lowbit) | (c >> (NB - 1) ? lo_up : lo))];
        if (FIRST) {
#pragma unroll
            for (int c = 0; c < N / 2; ++c) bitonic_cx(v[c], v[c ^ (N - 1)]);
        }
#pragma unroll
        for (int s = FIRST ? NB - 2 : NB - 1; s >= 0; --s) {
#pragma unroll
            for (int c = 0; c < N; ++c)
                if (!(c & (1 << s))) bitonic_cx(v[c], v[c | (1 << s)]);
        }
#pragma unroll
        for (int c = 0; c < N; ++c) keys[plan_pk(hi | (c << lowbit) | (c >> (NB - 1) ? lo_up : lo))] = v[c];
    }
    __syncthreads();
}

template <typename K>
__device__ inline void bitonic_sort_lds(K* keys, int P) {
    if (P >= 8) {                                  // stages k = 2, 4, 8 on eight consecutive keys, in registers
        for (int t = threadIdx.x; t < (P >> 3); t += PLAN_THREADS) {
            K v[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = keys[plan_pk(t * 8) + c];
#pragma unroll
            for (int m = 1; m <= 3; ++m) {
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    if (!(c & (1 << (m - 1)))) bitonic_cx(v[c], v[c ^ ((1 << m) - 1)]);
#pragma unroll
                for (int s = m - 2; s >= 0; --s) {
#pragma unroll
                    for (int c = 0; c < 8; ++c)
                        if (!(c & (1 << s))) bitonic_cx(v[c], v[c | (1 << s)]);
                }
            }
#pragma unroll
            for (int c = 0; c < 8; ++c) keys[plan_pk(t * 8) + c] = v[c];
        }
        __syncthreads();
    }
    for (int m = P >= 8 ? 4 : 1; (1 << m) <= P; ++m) {
        // sub-stage strides 2^(m-1) .. 1: the first pass takes what three-at-a-time leaves over, so that the last one
        // works on eight consecutive keys
        const int nb0 = m % 3 ? m % 3 : 3;
        if (nb0 == 3) bitonic_pass<K, 3, true>(keys, P, m - 1);
        else if (nb0 == 2) bitonic_pass<K, 2, true>(keys, P, m - 1);
        else bitonic_pass<K, 1, true>(keys, P, m - 1);
        for (int b = m - 1 - nb0; b >= 0; b -= 3) bitonic_pass<K, 3, false>(keys, P, b);
    }
}

// Exclusive prefix sum of one int per thread over the workgroup (wave scans + PLAN_THREADS / 64 wave totals in LDS).
__device__ inline int plan_block_scan(int v, int* scr, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int n = __shfl_up(inc, o, 64);
        if (lane >= o) inc += n;
    }
    if (lane == 63) scr[w] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < PLAN_THREADS / 64; ++i) {
        const int c = scr[i];
        base += i < w ? c : 0;
        tot += c;
    }
    __syncthreads();
    total = tot;
    return base + inc - v;
}

// keys[0..P) sorted, invalid = ~0.  Writes rows[], ptr[], list[] and returns the segment count.
template <typename K>
__device__ inline int plan_emit(const K* keys, int P, int32_t* rows, int32_t* ptr, int32_t* list, int* scan) {
    const int chunk = (P + PLAN_THREADS - 1) / PLAN_THREADS;
    const int e0 = threadIdx.x * chunk, e1 = min(e0 + chunk, P);
    int starts = 0, valid = 0;
    for (int e = e0; e < e1; ++e) {
        const K kx = keys[plan_pk(e)];
        if (kx == PlanKey<K>::INVALID) break;
        ++valid;
        if (e == 0 || PlanKey<K>::row(kx) != PlanKey<K>::row(keys[plan_pk(e - 1)])) ++starts;
    }
    int nseg, nvalid;
    int rank = plan_block_scan(starts, scan, nseg);
    plan_block_scan(valid, scan, nvalid);
    for (int e = e0; e < e1; ++e) {
        const K kx = keys[plan_pk(e)];
        if (kx == PlanKey<K>::INVALID) break;
        if (e == 0 || PlanKey<K>::row(kx) != PlanKey<K>::row(keys[plan_pk(e - 1)])) {
            rows[rank] = PlanKey<K>::row(kx);
            ptr[rank] = e;
            ++rank;
        }
        list[e] = PlanKey<K>::entry(kx);
    }
    if (threadIdx.x == 0) ptr[nseg] = nvalid;
    __syncthreads();
    return nseg;
}

// One side of one batch with keys of type K (LDS: P keys + the scan scratch); returns the side's row count.
// side 0: the L user keys (P / 2 slots); side 1: the 2 L item keys, positives then negatives.
template <typename K>
__device__ inline int plan_side(int side, const int32_t* iu, const int32_t* ip, const int32_t* in_, int64_t lo, int cnt,
                                int P, char* smem, int32_t* rows, int32_t* ptr, int32_t* list, int* scan) {
    K* keys = reinterpret_cast<K*>(smem);
    const int Ps = side == 0 && P > 2 ? P >> 1 : P;
    for (int e = threadIdx.x; e < Ps; e += PLAN_THREADS) {
        K kx = PlanKey<K>::INVALID;
        if (side == 0) {
            if (e < cnt) kx = PlanKey<K>::make((uint32_t)iu[lo + e], (unsigned)e, 0u);
        } else if (e < cnt) {
            kx = PlanKey<K>::make((uint32_t)ip[lo + e], (unsigned)e, 0u);
        } else if (e < 2 * cnt) {
            kx = PlanKey<K>::make((uint32_t)in_[lo + e - cnt], (unsigned)(e - cnt), 1u);
        }
        keys[plan_pk(e)] = kx;
    }
    __syncthreads();
    bitonic_sort_lds(keys, Ps);
    return plan_emit(keys, Ps, rows, ptr, list, scan);
}

__global__ __launch_bounds__(PLAN_THREADS) void bpr_plan_kernel(const int32_t* __restrict__ iu,
                                                                const int32_t* __restrict__ ip,
                                                                const int32_t* __restrict__ in_, int64_t n_rec,
                                                                int L, int P, int32_t* __restrict__ plans,
                                                                int64_t stride) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* scan = reinterpret_cast<int*>(smem + plan_padded_keys(P) * 8);      // behind the (padded) key area, sized for 64-bit keys
    const int side = blockIdx.y;                   // 0: user rows, 1: item rows -- one workgroup each
    const int64_t lo = (int64_t)blockIdx.x * L;
    const int cnt = (int)((n_rec - lo) < L ? (n_rec - lo) : L);
    int32_t* pl = plans + (int64_t)blockIdx.x * stride;
    const PlanSections<int32_t> ps = plan_sections(pl, L);

    // largest row id of this side decides the key width (block maximum: wave maxima through LDS)
    int mx = 0;
    for (int e = threadIdx.x; e < cnt; e += PLAN_THREADS) mx = max(mx, side == 0 ? iu[lo + e] : max(ip[lo + e], in_[lo + e]));
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = max(mx, __shfl_xor(mx, o, 64));
    if ((threadIdx.x & 63) == 0) scan[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = 0;
#pragma unroll
    for (int i = 0; i < PLAN_THREADS / 64; ++i) mx = max(mx, scan[i]);
    const bool narrow = mx < (1 << 17) && L <= 8192;
    __syncthreads();
    int32_t* rows = side == 0 ? ps.urow : ps.irow;
    int32_t* ptr = side == 0 ? ps.uptr : ps.iptr;
    int32_t* list = side == 0 ? ps.ulist : ps.ilist;
    const int n = narrow ? plan_side<uint32_t>(side, iu, ip, in_, lo, cnt, P, smem, rows, ptr, list, scan)
                         : plan_side<unsigned long long>(side, iu, ip, in_, lo, cnt, P, smem, rows, ptr, list, scan);
    if (threadIdx.x == 0) pl[side] = n;            // header: rows per side (the batch size follows in the heavy pass)
}

// Second launch of the LDS builder, one workgroup per plan, once both sides' rows are in place: the plan header and the
// heavy rows, ascending (a fixed order: the one-launch MF step sums per-block partials, and which block takes which heavy
// row follows the list) -- count per thread chunk, scan of the counts, ordered write.
__global__ __launch_bounds__(PLAN_THREADS) void bpr_plan_heavy_kernel(int L, int32_t* __restrict__ plans, int64_t stride) {
    __shared__ int scan[PLAN_THREADS / 64];
    int32_t* pl = plans + (int64_t)blockIdx.x * stride;
    const int nu = pl[0], ni = pl[1];
    const PlanSections<int32_t> ps = plan_sections(pl, L);
    const int rchunk = (nu + ni + PLAN_THREADS - 1) / PLAN_THREADS;
    const int r0 = threadIdx.x * rchunk, r1 = min(r0 + rchunk, nu + ni);
    int nh = 0;
    for (int r = r0; r < r1; ++r) nh += plan_row_heavy(ps.uptr, ps.iptr, nu, r);
    __syncthreads();
    int n_heavy;
    int w = plan_block_scan(nh, scan, n_heavy);
    if (threadIdx.x == 0) {
        pl[0] = nu;
        pl[1] = ni;
        pl[2] = (int32_t)L;
        ps.heavy[0] = n_heavy;
    }
    for (int r = r0; r < r1; ++r)
        if (plan_row_heavy(ps.uptr, ps.iptr, nu, r)) ps.heavy[1 + w++] = r;
}

// Heavy lists for plans whose row lists were built by several workgroups (crh_bpr_plan_build_large: up to 3 x 524288
// rows per plan).  Two passes over HV_BLOCKS chunks per plan: count, then ordered write.
constexpr int HV_BLOCKS = 64, HV_THREADS = 256;

__global__ __launch_bounds__(HV_THREADS) void plan_heavy_pass_kernel(int32_t* plans, int64_t stride, int32_t* counts,
                                                                      int write) {
    __shared__ int scan[HV_THREADS];
    __shared__ int base_s;
    int32_t* pl = plans + (int64_t)blockIdx.y * stride;
    const PlanSections<int32_t> ps = plan_sections(pl, pl[2]);
    const int nu = pl[0], ni = pl[1], n = nu + ni;
    const int per_block = (n + HV_BLOCKS - 1) / HV_BLOCKS;
    const int b0 = blockIdx.x * per_block, b1 = min(b0 + per_block, n);
    const int rc = (max(b1 - b0, 0) + HV_THREADS - 1) / HV_THREADS;
    const int t0 = b0 + threadIdx.x * rc, t1 = min(t0 + rc, b1);
    int nh = 0;
    for (int r = t0; r < t1; ++r) nh += plan_row_heavy(ps.uptr, ps.iptr, nu, r);
    scan[threadIdx.x] = nh;
    __syncthreads();
    int32_t* cnt = counts + (int64_t)blockIdx.y * HV_BLOCKS;
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int i = 0; i < HV_THREADS; ++i) {
            const int c = scan[i];
            scan[i] = acc;
            acc += c;
        }
        if (!write) {
            cnt[blockIdx.x] = acc;
        } else {
            int base = 0, total = 0;
            for (int i = 0; i < HV_BLOCKS; ++i) {
                if (i < (int)blockIdx.x) base += cnt[i];
                total += cnt[i];
            }
            base_s = base;
            if (blockIdx.x == 0) ps.heavy[0] = total;
        }
    }
    if (!write) return;
    __syncthreads();
    int w = 1 + base_s + scan[threadIdx.x];
    for (int r = t0; r < t1; ++r)
        if (plan_row_heavy(ps.uptr, ps.iptr, nu, r)) ps.heavy[w++] = r;
}

// ---------------------------------------------------------------- plan builder for batches beyond the LDS sort
// Batches above 8 192 triples (S-TRAIN-XL: 65 536) do not fit one workgroup's LDS.  Same result, several workgroups
// per batch: (1) chunks of LP_CHUNK keys are sorted in LDS (bitonic, 64-bit keys row << 31 | role << 30 | entry);
// (2) log2(chunks) merge passes in global memory, every thread producing LP_VT consecutive outputs of one merged pair
// from its merge-path split (keys are unique, so there are no ties to order); (3) segment starts are counted per block,
// each block sums the counts of the blocks before it, and rows / offsets / lists are written in place; (4) the heavy
// lists by plan_heavy_pass_kernel.  grid.y = batch, so an epoch's plans are a handful of launches.
constexpr int LP_CHUNK = 8192, LP_VT = 8, LP_EMIT = 4096, LP_MAX_EBLOCKS = 256;
typedef unsigned long long lpkey;

__device__ __forceinline__ lpkey lp_key(const int32_t* iu, const int32_t* ip, const int32_t* in_, int64_t lo, int cnt,
                                        int item_side, int64_t e) {
    if (!item_side) return e < cnt ? PlanKey<lpkey>::make((uint32_t)iu[lo + e], (unsigned)e, 0u) : PlanKey<lpkey>::INVALID;
    if (e < cnt) return PlanKey<lpkey>::make((uint32_t)ip[lo + e], (unsigned)e, 0u);
    if (e < 2 * (int64_t)cnt) return PlanKey<lpkey>::make((uint32_t)in_[lo + e - cnt], (unsigned)(e - cnt), 1u);
    return PlanKey<lpkey>::INVALID;
}

__global__ __launch_bounds__(PLAN_THREADS) void plan_chunk_sort_kernel(const int32_t* __restrict__ iu,
                                                                        const int32_t* __restrict__ ip,
                                                                        const int32_t* __restrict__ in_, int64_t n_rec,
                                                                        int64_t L, int item_side, int64_t P,
                                                                        lpkey* __restrict__ keys) {
    __shared__ lpkey sk[plan_padded_keys(LP_CHUNK)];
    const int64_t lo = (int64_t)blockIdx.y * L;
    const int cnt = (int)((n_rec - lo) < L ? (n_rec - lo) : L);
    const int64_t c0 = (int64_t)blockIdx.x * LP_CHUNK;
    for (int e = threadIdx.x; e < LP_CHUNK; e += PLAN_THREADS) sk[plan_pk(e)] = lp_key(iu, ip, in_, lo, cnt, item_side, c0 + e);
    __syncthreads();
    bitonic_sort_lds(sk, LP_CHUNK);
    lpkey* out = keys + (int64_t)blockIdx.y * P + c0;
    for (int e = threadIdx.x; e < LP_CHUNK; e += PLAN_THREADS) out[e] = sk[plan_pk(e)];
}

__global__ __launch_bounds__(256) void plan_merge_pass_kernel(const lpkey* __restrict__ src, lpkey* __restrict__ dst,
                                                              int64_t P, int64_t run) {
    const int64_t o0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * LP_VT;
    if (o0 >= P) return;
    const lpkey* a = src + (int64_t)blockIdx.y * P + (o0 / (2 * run)) * (2 * run);
    const lpkey* b = a + run;
    const int64_t d = o0 % (2 * run);
    int64_t lo = d > run ? d - run : 0, hi = d < run ? d : run;
    while (lo < hi) {                       // merge path: the first i with a[i] >= b[d - 1 - i]
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] < b[d - 1 - mid]) lo = mid + 1;
        else hi = mid;
    }
    int64_t i = lo, j = d - lo;
    lpkey* out = dst + (int64_t)blockIdx.y * P + o0;
    lpkey av = i < run ? a[i] : PlanKey<lpkey>::INVALID, bv = j < run ? b[j] : PlanKey<lpkey>::INVALID;
#pragma unroll
    for (int k = 0; k < LP_VT; ++k) {
        const bool take_a = j >= run || (i < run && av < bv);
        out[k] = take_a ? av : bv;
        if (take_a) { ++i; av = i < run ? a[i] : PlanKey<lpkey>::INVALID; }
        else { ++j; bv = j < run ? b[j] : PlanKey<lpkey>::INVALID; }
    }
}

// write = 0: counts[batch][block] = segment starts of the block's LP_EMIT keys; write = 1: rows / offsets / list.
__global__ __launch_bounds__(PLAN_THREADS) void plan_emit_large_kernel(const lpkey* __restrict__ keys, int64_t P,
                                                                        int64_t n_rec, int64_t L, int item_side,
                                                                        int32_t* __restrict__ plans, int64_t stride,
                                                                        int32_t* __restrict__ counts, int n_eblocks,
                                                                        int write) {
    __shared__ int scan[PLAN_THREADS];
    __shared__ int base_s, total_s;
    const int64_t lo = (int64_t)blockIdx.y * L;
    const int cnt = (int)((n_rec - lo) < L ? (n_rec - lo) : L);
    const int64_t nvalid = item_side ? 2 * (int64_t)cnt : cnt;
    const lpkey* k = keys + (int64_t)blockIdx.y * P;
    int32_t* pl = plans + (int64_t)blockIdx.y * stride;
    const PlanSections<int32_t> ps = plan_sections(pl, L);
    int32_t* rows = item_side ? ps.irow : ps.urow;
    int32_t* ptr = item_side ? ps.iptr : ps.uptr;
    int32_t* list = item_side ? ps.ilist : ps.ulist;
    constexpr int PER = LP_EMIT / PLAN_THREADS;
    const int64_t e0 = (int64_t)blockIdx.x * LP_EMIT + (int64_t)threadIdx.x * PER;
    int starts = 0;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int64_t e = e0 + q;
        if (e < nvalid && (e == 0 || PlanKey<lpkey>::row(k[e]) != PlanKey<lpkey>::row(k[e - 1]))) ++starts;
    }
    scan[threadIdx.x] = starts;
    __syncthreads();
    for (int off = 1; off < PLAN_THREADS; off <<= 1) {      // inclusive scan of the per-thread counts
        const int v = (int)threadIdx.x >= off ? scan[threadIdx.x - off] : 0;
        __syncthreads();
        scan[threadIdx.x] += v;
        __syncthreads();
    }
    int32_t* cb = counts + (int64_t)blockIdx.y * LP_MAX_EBLOCKS;
    if (!write) {
        if (threadIdx.x == PLAN_THREADS - 1) cb[blockIdx.x] = scan[PLAN_THREADS - 1];
        return;
    }
    if (threadIdx.x == 0) {
        int base = 0, total = 0;
        for (int b = 0; b < n_eblocks; ++b) {
            if (b < (int)blockIdx.x) base += cb[b];
            total += cb[b];
        }
        base_s = base;
        total_s = total;
    }
    __syncthreads();
    int rank = base_s + scan[threadIdx.x] - starts;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int64_t e = e0 + q;
        if (e >= nvalid) break;
        const lpkey kx = k[e];
        if (e == 0 || PlanKey<lpkey>::row(kx) != PlanKey<lpkey>::row(k[e - 1])) {
            rows[rank] = PlanKey<lpkey>::row(kx);
            ptr[rank] = (int32_t)e;
            ++rank;
        }
        list[e] = PlanKey<lpkey>::entry(kx);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ptr[total_s] = (int32_t)nvalid;
        pl[item_side ? 1 : 0] = total_s;
        pl[2] = (int32_t)L;
    }
}

int64_t lp_padded(int64_t width) {
    const int64_t c = (width + LP_CHUNK - 1) / LP_CHUNK;
    int64_t p = 1;
    while (p < c) p <<= 1;
    return p * LP_CHUNK;
}
size_t lp_align(size_t x) { return (x + 255) & ~(size_t)255; }

// (Re)build the heavy-row lists of n_batches plans whose header and row lists are in place.
size_t plan_heavy_workspace_bytes(int64_t n_batches) {
    return n_batches > 0 ? (size_t)n_batches * HV_BLOCKS * sizeof(int32_t) : 0;
}

int plan_heavy_lists(int32_t* plans, int64_t n_batches, int64_t layout_batch, void* workspace, size_t workspace_bytes,
                     void* stream) {
    CRH_CHECK_ARG(plans && n_batches > 0 && n_batches <= 65535 && layout_batch > 0, "crh_bpr_plan_heavy_lists: bad arguments");
    if (!workspace || workspace_bytes < plan_heavy_workspace_bytes(n_batches)) {
        crh_set_error("crh_bpr_plan_heavy_lists: workspace %zu < %zu bytes", workspace_bytes,
                      plan_heavy_workspace_bytes(n_batches));
        return CRH_ERR_WS;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    for (int pass = 0; pass < 2; ++pass) {
        hipLaunchKernelGGL(plan_heavy_pass_kernel, dim3(HV_BLOCKS, (unsigned)n_batches), dim3(HV_THREADS), 0, st, plans,
                           plan_ints(layout_batch), reinterpret_cast<int32_t*>(workspace), pass);
        CRH_HIP(hipGetLastError());
    }
    return CRH_OK;
}

}  // namespace

extern "C" int64_t crh_bpr_plan_ints(int64_t batch) { return batch > 0 ? plan_ints(batch) : 0; }
extern "C" int crh_bpr_heavy_threshold(void) { return BPR_HEAVY; }

// HOST function: reverse index of one batch of triples (see bpr_bwd_rows_kernel).  Item-side
// gradients of positives and negatives land in the SAME table (grad_pos == grad_neg).
extern "C" int crh_bpr_plan_build_host(const int32_t* user_idx_host, const int32_t* pos_idx_host,
                                       const int32_t* neg_idx_host, int64_t batch, int64_t layout_batch,
                                       int32_t* plan_out_host) {
    CRH_CHECK_ARG(user_idx_host && pos_idx_host && neg_idx_host && plan_out_host && batch > 0,
                  "crh_bpr_plan_build_host: bad arguments");
    CRH_CHECK_ARG(layout_batch >= batch && layout_batch < (1 << 30), "crh_bpr_plan_build_host: bad layout batch");
    const int64_t B = batch, L = layout_batch;
    int32_t* pl = plan_out_host;
    const PlanSections<int32_t> ps = plan_sections(pl, L);
    pl[2] = (int32_t)L;
    std::vector<uint64_t> keys((size_t)2 * B);
    for (int64_t b = 0; b < B; ++b) keys[b] = ((uint64_t)(uint32_t)user_idx_host[b] << 32) | (uint32_t)b;
    std::sort(keys.begin(), keys.begin() + B);
    int nu = 0;
    for (int64_t e = 0; e < B; ++e) {
        const int32_t row = (int32_t)(keys[e] >> 32);
        if (e == 0 || row != ps.urow[nu - 1]) { ps.urow[nu] = row; ps.uptr[nu] = (int32_t)e; ++nu; }
        ps.ulist[e] = (int32_t)(keys[e] & 0xffffffffu);
    }
    ps.uptr[nu] = (int32_t)B;
    for (int64_t b = 0; b < B; ++b) {
        keys[2 * b] = ((uint64_t)(uint32_t)pos_idx_host[b] << 32) | (uint32_t)b;
        keys[2 * b + 1] = ((uint64_t)(uint32_t)neg_idx_host[b] << 32) | (uint32_t)b | (1u << 30);
    }
    std::sort(keys.begin(), keys.end());      // inside a row: positives (ascending b), then negatives
    int ni = 0;
    for (int64_t e = 0; e < 2 * B; ++e) {
        const int32_t row = (int32_t)(keys[e] >> 32);
        if (e == 0 || row != ps.irow[ni - 1]) { ps.irow[ni] = row; ps.iptr[ni] = (int32_t)e; ++ni; }
        ps.ilist[e] = (int32_t)(keys[e] & 0xffffffffu);
    }
    ps.iptr[ni] = (int32_t)(2 * B);
    pl[0] = nu;
    pl[1] = ni;
    int nh = 0;
    for (int r = 0; r < nu + ni; ++r)
        if (plan_row_heavy(ps.uptr, ps.iptr, nu, r)) ps.heavy[1 + nh++] = r;
    ps.heavy[0] = nh;
    return CRH_OK;
}

// Device: plans of every batch of an epoch in one launch (batch_size <= 8192; the sort runs in LDS).
extern "C" int crh_bpr_plan_build(const int32_t* user_idx, const int32_t* pos_idx, const int32_t* neg_idx,
                                  int64_t n_records, int64_t batch_size, int32_t* plans_out, void* stream) {
    CRH_CHECK_ARG(user_idx && pos_idx && neg_idx && plans_out && n_records > 0, "crh_bpr_plan_build: bad arguments");
    CRH_CHECK_ARG(batch_size >= 1 && batch_size <= 8192, "crh_bpr_plan_build: batch_size=%lld outside 1..8192 "
                  "(larger batches: crh_bpr_plan_build_large)", (long long)batch_size);
    int P = 2;
    while (P < 2 * batch_size) P <<= 1;
    const size_t lds = plan_padded_keys(P) * 8 + (2 * PLAN_THREADS + 2) * sizeof(int);
    const int64_t nb = (n_records + batch_size - 1) / batch_size;
    if (lds > 64 * 1024)
        CRH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(bpr_plan_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(bpr_plan_kernel, dim3((unsigned)nb, 2), dim3(PLAN_THREADS), lds,
                       reinterpret_cast<hipStream_t>(stream), user_idx, pos_idx, neg_idx, n_records, (int)batch_size,
                       P, plans_out, plan_ints(batch_size));
    CRH_HIP(hipGetLastError());
    hipLaunchKernelGGL(bpr_plan_heavy_kernel, dim3((unsigned)nb), dim3(PLAN_THREADS), 0,
                       reinterpret_cast<hipStream_t>(stream), (int)batch_size, plans_out, plan_ints(batch_size));
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

// Workspace of crh_bpr_plan_build_large: two key buffers of the (padded) item side per batch, the per-block segment
// counts, the heavy-list counts.
extern "C" size_t crh_bpr_plan_build_large_workspace_bytes(int64_t n_records, int64_t batch_size) {
    if (n_records <= 0 || batch_size <= 0) return 0;
    const int64_t nb = (n_records + batch_size - 1) / batch_size;
    return 2 * lp_align((size_t)nb * lp_padded(2 * batch_size) * sizeof(lpkey)) +
           lp_align((size_t)nb * LP_MAX_EBLOCKS * sizeof(int32_t)) + lp_align(plan_heavy_workspace_bytes(nb));
}

// Device: plans of every batch of an epoch for ANY batch size up to 524 288 (several workgroups per batch: chunk sorts in
// LDS, merge passes in global memory; see plan_chunk_sort_kernel).  Same layout and contents as crh_bpr_plan_build.
extern "C" int crh_bpr_plan_build_large(const int32_t* user_idx, const int32_t* pos_idx, const int32_t* neg_idx,
                                        int64_t n_records, int64_t batch_size, int32_t* plans_out, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    CRH_CHECK_ARG(user_idx && pos_idx && neg_idx && plans_out && n_records > 0, "crh_bpr_plan_build_large: bad arguments");
    CRH_CHECK_ARG(batch_size >= 1 && lp_padded(2 * batch_size) <= (int64_t)LP_EMIT * LP_MAX_EBLOCKS,
                  "crh_bpr_plan_build_large: batch_size=%lld outside 1..%lld", (long long)batch_size,
                  (long long)LP_EMIT * LP_MAX_EBLOCKS / 2);
    const int64_t L = batch_size, nb = (n_records + L - 1) / L;
    CRH_CHECK_ARG(nb <= 65535, "crh_bpr_plan_build_large: %lld batches in one call (at most 65535)", (long long)nb);
    const size_t need = crh_bpr_plan_build_large_workspace_bytes(n_records, batch_size);
    if (!workspace || workspace_bytes < need) {
        crh_set_error("crh_bpr_plan_build_large: workspace %zu < %zu bytes", workspace_bytes, need);
        return CRH_ERR_WS;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t key_b = lp_align((size_t)nb * lp_padded(2 * L) * sizeof(lpkey));
    char* wsp = reinterpret_cast<char*>(workspace);
    lpkey* buf[2] = {reinterpret_cast<lpkey*>(wsp), reinterpret_cast<lpkey*>(wsp + key_b)};
    int32_t* counts = reinterpret_cast<int32_t*>(wsp + 2 * key_b);
    void* heavy_ws = wsp + 2 * key_b + lp_align((size_t)nb * LP_MAX_EBLOCKS * sizeof(int32_t));
    const int64_t stride = plan_ints(L);
    CRH_HIP(hipMemsetAsync(plans_out, 0, (size_t)nb * stride * sizeof(int32_t), st));
    for (int side = 0; side < 2; ++side) {
        const int64_t P = lp_padded(side ? 2 * L : L);
        hipLaunchKernelGGL(plan_chunk_sort_kernel, dim3((unsigned)(P / LP_CHUNK), (unsigned)nb), dim3(PLAN_THREADS), 0, st,
                           user_idx, pos_idx, neg_idx, n_records, L, side, P, buf[0]);
        CRH_HIP(hipGetLastError());
        int cur = 0;
        for (int64_t run = LP_CHUNK; run < P; run <<= 1) {
            hipLaunchKernelGGL(plan_merge_pass_kernel, dim3((unsigned)((P / LP_VT + 255) / 256), (unsigned)nb), dim3(256), 0,
                               st, buf[cur], buf[cur ^ 1], P, run);
            CRH_HIP(hipGetLastError());
            cur ^= 1;
        }
        const int n_eblocks = (int)((P + LP_EMIT - 1) / LP_EMIT);
        for (int write = 0; write < 2; ++write) {
            hipLaunchKernelGGL(plan_emit_large_kernel, dim3((unsigned)n_eblocks, (unsigned)nb), dim3(PLAN_THREADS), 0, st,
                               buf[cur], P, n_records, L, side, plans_out, stride, counts, n_eblocks, write);
            CRH_HIP(hipGetLastError());
        }
    }
    return plan_heavy_lists(plans_out, nb, L, heavy_ws, plan_heavy_workspace_bytes(nb), stream);
}
