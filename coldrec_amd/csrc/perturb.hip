// The layer perturbation of SimGCL / XSimGCL (model/SimGCL.py:106-108, model/XSimGCL.py:112-114):
//     y += sign(y) * normalize(rand_like(y), dim=-1) * eps
// applied in place to one layer output of the propagation, with the layer mean's running sum fused in (the mean must see
// the perturbed rows).  One row is handled by one lane group of d/4 lanes (16 bytes per lane, padded to a power of two
// of lanes so that the row norm is an xor-shuffle tree inside the group): no LDS, no atomics, one read and one write of
// y plus the accumulator -- an HBM-bound streaming kernel.
// The uniforms come either from a caller's buffer (parity with the reference: the host draws them from torch's CPU
// generator) or from Philox4x32-10 in registers, counter = (row * d/4 + column group, draw), key = seed:
// crh_noise_uniform_f32 writes exactly those uniforms.
#include <math.h>

#include "crh_common.h"

namespace {

constexpr unsigned PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;
constexpr int PERTURB_THREADS = 256;
constexpr int64_t PERTURB_MAX_BLOCKS = 1 << 20;

// the four uniforms in [0, 1) of column group g (columns 4 * (g % (d/4)) .. + 3 of row g / (d/4)) of draw `draw`
__device__ __forceinline__ f32x4 philox_uniform4(uint64_t g, uint64_t draw, uint64_t seed) {
    unsigned c0 = (unsigned)g, c1 = (unsigned)(g >> 32), c2 = (unsigned)draw, c3 = (unsigned)(draw >> 32);
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
        const unsigned hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    const float s = 1.0f / 16777216.0f;          // 2^-24: (word >> 8) is exact in fp32
    f32x4 u;
    u.x = (float)(c0 >> 8) * s;
    u.y = (float)(c1 >> 8) * s;
    u.z = (float)(c2 >> 8) * s;
    u.w = (float)(c3 >> 8) * s;
    return u;
}

__device__ __forceinline__ uint64_t draw_index(const int64_t* draw_dev, int64_t draw_offset) {
    return (uint64_t)((draw_dev ? draw_dev[0] : 0) + draw_offset);
}

__global__ __launch_bounds__(PERTURB_THREADS) void noise_uniform_kernel(float* __restrict__ out, int64_t n_groups, uint64_t seed,
                                                                        const int64_t* __restrict__ draw_dev, int64_t draw_offset) {
    const uint64_t draw = draw_index(draw_dev, draw_offset);
    for (int64_t g = (int64_t)blockIdx.x * PERTURB_THREADS + threadIdx.x; g < n_groups; g += (int64_t)gridDim.x * PERTURB_THREADS)
        reinterpret_cast<f32x4*>(out)[g] = philox_uniform4((uint64_t)g, draw, seed);
}

// G = lanes of a lane group (power of two >= d/4); lanes d/4 .. G-1 of a group idle (they add 0 to the norm).
template <int G>
__global__ __launch_bounds__(PERTURB_THREADS) void perturb_rows_kernel(float* y, int64_t n_rows, int d4, float eps,
                                                                       const float* __restrict__ noise, uint64_t seed,
                                                                       const int64_t* __restrict__ draw_dev, int64_t draw_offset,
                                                                       const float* acc_in, float s_in, float* acc_out, float s_out) {
    // every product, quotient and sum rounded on its own, as the separate ATen ops of the reference do
#pragma clang fp contract(off)
    constexpr int ROWS = PERTURB_THREADS / G;                  // rows of one block and pass
    const int lane = threadIdx.x % G, sub = threadIdx.x / G;
    const uint64_t draw = noise ? 0 : draw_index(draw_dev, draw_offset);
    // the loop bound is the same for the whole block: all 64 lanes of a wave reach every shuffle
    for (int64_t base = (int64_t)blockIdx.x * ROWS; base < n_rows; base += (int64_t)gridDim.x * ROWS) {
        const int64_t row = base + sub;
        const bool active = row < n_rows && lane < d4;
        const int64_t g = row * d4 + lane;                     // column group = index of the row's 16-byte slice
        f32x4 r = {0.f, 0.f, 0.f, 0.f};
        if (active) r = noise ? reinterpret_cast<const f32x4*>(noise)[g] : philox_uniform4((uint64_t)g, draw, seed);
        float ss = (r.x * r.x + r.y * r.y) + (r.z * r.z + r.w * r.w);
#pragma unroll
        for (int off = G / 2; off >= 1; off >>= 1) ss += __shfl_xor(ss, off);
        if (!active) continue;
        const float nrm = fmaxf(sqrtf(ss), 1e-12f);            // F.normalize's clamp
        f32x4 v = reinterpret_cast<const f32x4*>(y)[g];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float sg = v[c] > 0.f ? 1.f : (v[c] < 0.f ? -1.f : 0.f);
            v[c] = v[c] + (sg * (r[c] / nrm)) * eps;
        }
        reinterpret_cast<f32x4*>(y)[g] = v;
        if (acc_out) {
            f32x4 a = {0.f, 0.f, 0.f, 0.f};
            if (acc_in) a = reinterpret_cast<const f32x4*>(acc_in)[g];
#pragma unroll
            for (int c = 0; c < 4; ++c) a[c] = (a[c] * s_in + v[c]) * s_out;
            reinterpret_cast<f32x4*>(acc_out)[g] = a;
        }
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int crh_noise_uniform_f32(float* out, int64_t n_rows, int d, uint64_t seed, const int64_t* draw_dev,
                                     int64_t draw_offset, void* stream) {
    CRH_CHECK_ARG(out && n_rows >= 0, "crh_noise_uniform_f32: NULL pointer / negative row count");
    CRH_CHECK_ARG(d % 4 == 0 && d >= 4 && d <= 256, "crh_noise_uniform_f32: d = %d must be a multiple of 4 in [4, 256]", d);
    CRH_CHECK_ARG(aligned16(out), "crh_noise_uniform_f32: out must be 16-byte aligned");
    if (n_rows == 0) return CRH_OK;
    const int64_t n_groups = n_rows * (d / 4);
    int64_t blocks = (n_groups + PERTURB_THREADS - 1) / PERTURB_THREADS;
    if (blocks > PERTURB_MAX_BLOCKS) blocks = PERTURB_MAX_BLOCKS;
    hipLaunchKernelGGL(noise_uniform_kernel, dim3((unsigned)blocks), dim3(PERTURB_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       out, n_groups, seed, draw_dev, draw_offset);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

extern "C" int crh_perturb_rows_f32(float* y, int64_t n_rows, int d, float eps, const float* noise, uint64_t seed,
                                    const int64_t* draw_dev, int64_t draw_offset, const float* acc_in, float s_in,
                                    float* acc_out, float s_out, void* stream) {
    CRH_CHECK_ARG(y && n_rows >= 0, "crh_perturb_rows_f32: NULL pointer / negative row count");
    CRH_CHECK_ARG(d % 4 == 0 && d >= 4 && d <= 256, "crh_perturb_rows_f32: d = %d must be a multiple of 4 in [4, 256]", d);
    CRH_CHECK_ARG(!(acc_in && !acc_out), "crh_perturb_rows_f32: acc_in given without acc_out");
    CRH_CHECK_ARG(aligned16(y) && aligned16(noise) && aligned16(acc_in) && aligned16(acc_out),
                  "crh_perturb_rows_f32: y, noise and the accumulators must be 16-byte aligned");
    if (n_rows == 0) return CRH_OK;
    const int d4 = d / 4;
    int G = 1;
    while (G < d4) G <<= 1;
    const int rows_per_block = PERTURB_THREADS / G;
    int64_t blocks = (n_rows + rows_per_block - 1) / rows_per_block;
    if (blocks > PERTURB_MAX_BLOCKS) blocks = PERTURB_MAX_BLOCKS;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define CRH_PERTURB_LAUNCH(GG)                                                                                            \
    case GG:                                                                                                              \
        hipLaunchKernelGGL(perturb_rows_kernel<GG>, dim3((unsigned)blocks), dim3(PERTURB_THREADS), 0, st, y, n_rows, d4, \
                           eps, noise, seed, draw_dev, draw_offset, acc_in, s_in, acc_out, s_out);                        \
        break;
    switch (G) {
        CRH_PERTURB_LAUNCH(1)
        CRH_PERTURB_LAUNCH(2)
        CRH_PERTURB_LAUNCH(4)
        CRH_PERTURB_LAUNCH(8)
        CRH_PERTURB_LAUNCH(16)
        CRH_PERTURB_LAUNCH(32)
        CRH_PERTURB_LAUNCH(64)
    }
#undef CRH_PERTURB_LAUNCH
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}
