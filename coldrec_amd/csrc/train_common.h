// What the row kernels of the BPR / MF training path share (bpr.hip, optim.hip, mf_step.hip): the lane-group picker and
// its dispatcher, the group and block sums, and the reductions that the three-launch step (bpr_bwd_rows_kernel) and the
// one-launch step (mf_step_kernel) must compute with the same bits -- batch totals from block partials, norms to
// regulariser coefficients, a heavy row's chunk split and its cross-group sum tree.  Each exists here once.
// The fused-loss kernels have their own helpers (loss_common.h); the two headers are not meant to meet.
#pragma once
#include <math.h>

#include <type_traits>

#include "crh_common.h"

constexpr int BPR_THREADS = 256;

// lanes per table row: the smallest power of two that covers the row's d / 4 16-byte slices, at most a wave
inline int pick_group(int d) {
    const int nvec = d / 4;
    int g = 1;
    while (g < nvec && g < 64) g <<= 1;
    return g;
}

template <typename F>
int dispatch_group(int g, F&& f) {
    switch (g) {
        case 1: return f(std::integral_constant<int, 1>());
        case 2: return f(std::integral_constant<int, 2>());
        case 4: return f(std::integral_constant<int, 4>());
        case 8: return f(std::integral_constant<int, 8>());
        case 16: return f(std::integral_constant<int, 16>());
        case 32: return f(std::integral_constant<int, 32>());
        default: return f(std::integral_constant<int, 64>());
    }
}

template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int off = G / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, G);
    return v;
}

__device__ __forceinline__ float block_sum(float v, float* red) {
    // deterministic: wave butterfly then fixed-order sum of the 4 wave results
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ float dot4(const f32x4& a, const f32x4& b) {
#pragma clang fp contract(off)      // the same bits wherever a score difference is recomputed
    return ((a.x * b.x + a.y * b.y) + a.z * b.z) + a.w * b.w;
}

// Batch sums (u^2, p^2, n^2, loss) from n per-block partials of four floats, in every thread of a BPR_THREADS block: the
// four sums in ONE pass over the partials (16-byte loads) and one reduction -- component by component the arithmetic of
// block_sum over a thread-strided sum.  Every block of a launch reduces the same partials in the same order, so all get
// identical, deterministic totals.  red4 is written ONCE per launch (one call per kernel), so no thread can still be
// reading it when the wave leaders write: no barrier is needed before the write, only the one before the reads.
__device__ __forceinline__ f32x4 partials_total(const float* partials, int n) {
    __shared__ f32x4 red4[4];
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < n; i += BPR_THREADS) {
        const f32x4 x = reinterpret_cast<const f32x4*>(partials)[i];
        s.x += x.x; s.y += x.y; s.z += x.z; s.w += x.w;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        s.x += __shfl_xor(s.x, off); s.y += __shfl_xor(s.y, off);
        s.z += __shfl_xor(s.z, off); s.w += __shfl_xor(s.w, off);
    }
    if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = s;
    __syncthreads();
    const f32x4 t0 = red4[0], t1 = red4[1], t2 = red4[2], t3 = red4[3];
    f32x4 tot;
    tot.x = (t0.x + t1.x) + (t2.x + t3.x);
    tot.y = (t0.y + t1.y) + (t2.y + t3.y);
    tot.z = (t0.z + t1.z) + (t2.z + t3.z);
    tot.w = (t0.w + t1.w) + (t2.w + t3.w);
    return tot;
}

// What a backward needs of the batch sums: 1 / B, the coefficients of the regulariser's gradient
//   d(reg*|X|_F/B)/dX = reg * X / (B*|X|_F)   (0 at X = 0, as autograd returns)
// for the user, positive and negative rows, and the regulariser's value l2 = reg * (|U| + |P| + |N|) / B for the caller
// that reports it (which loss goes where differs between the kernels and stays with them).
struct BwdCoef {
    float invB, cu, cp, cn, l2;
};

__device__ __forceinline__ BwdCoef bwd_coef(const f32x4& tot, float reg, float invB) {
    BwdCoef k;
    k.invB = invB;
    const float nu_ = sqrtf(tot.x), np_ = sqrtf(tot.y), nn = sqrtf(tot.z);
    k.l2 = reg * (nu_ * k.invB + np_ * k.invB + nn * k.invB);
    k.cu = nu_ > 0.f ? reg * k.invB / nu_ : 0.f;
    k.cp = np_ > 0.f ? reg * k.invB / np_ : 0.f;
    k.cn = nn > 0.f ? reg * k.invB / nn : 0.f;
    return k;
}

// A heavy row is summed by one whole block: its BPR_THREADS / G lane groups split the row's entries [r0, r1) into
// contiguous chunks (a multiple of 4 entries each, the gather depth of the entry loops); this lane group's is [e0, e1),
// empty if e0 >= r1.
template <int G>
__device__ __forceinline__ void heavy_row_chunk(int r0, int r1, int& e0, int& e1) {
    constexpr int NGB = BPR_THREADS / G;
    int chunk = (r1 - r0 + NGB - 1) / NGB;
    chunk = (chunk + 3) & ~3;
    e0 = r0 + (int)(threadIdx.x / G) * chunk;
    e1 = e0 + chunk < r1 ? e0 + chunk : r1;
}

// ... and the lane groups' partial sums meet in a fixed order: a shuffle tree over the groups of a wave, the 4 waves
// through LDS.  Returns the row's sum (slice threadIdx.x) on the lanes threadIdx.x < G; the other lanes get the sum of a
// slice that is not theirs and drop it.  Two barriers: every thread of the block calls it, the same number of times.
// (A form that returns a flag and hands the sum out through a reference costs mf_step_kernel 4 to 12 VGPRs.)
template <int G>
__device__ __forceinline__ f32x4 heavy_row_sum(f32x4 acc, f32x4 (*wsum)[G]) {
    const int lig = threadIdx.x % G;
#pragma unroll
    for (int off = G; off < 64; off <<= 1) {
        acc.x += __shfl_down(acc.x, off);
        acc.y += __shfl_down(acc.y, off);
        acc.z += __shfl_down(acc.z, off);
        acc.w += __shfl_down(acc.w, off);
    }
    __syncthreads();
    if ((threadIdx.x & 63) < G) wsum[threadIdx.x >> 6][lig] = acc;
    __syncthreads();
    const f32x4 t0 = wsum[0][lig], t1 = wsum[1][lig], t2 = wsum[2][lig], t3 = wsum[3][lig];
    f32x4 r;
    r.x = (t0.x + t1.x) + (t2.x + t3.x);
    r.y = (t0.y + t1.y) + (t2.y + t3.y);
    r.z = (t0.z + t1.z) + (t2.z + t3.z);
    r.w = (t0.w + t1.w) + (t2.w + t3.w);
    return r;
}
