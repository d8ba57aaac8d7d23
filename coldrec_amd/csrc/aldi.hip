// The loss of ALDI (reference model/ALDI.py:47-82), forward and backward in one call.  Per record b of the batch: the
// user u_b, the positive p_b, the negative n_b; the frozen teacher rows Ur = U[u_b], Pr = V[p_b], Nr = V[n_b]; the student
// towers' outputs gu_b, gp_b, gn_b; the weight wi = w[p_b].  With sp = <gu, gp>, sn = <gu, gn>, tp = <Ur, Pr>,
// tn = <Ur, Nr>, bce(x, z) = max(x, 0) - x z + log1p(exp(-|x|)) and every mean over the B records:
//
//   L_bpr  = mean(-log(1e-5 + sigmoid(sp - sn)))
//   L_rate = gamma mean(|tp - sp| + |tn - sn|)                                  (d|x| / dx = 0 at 0)
//   L_rank = alpha mean(wi bce(sp - sn, sigmoid(tp - tn)))
//   L_iden = beta  mean(wi bce(|gp|^2 - <gp, mean_j gn_j>, sigmoid(|Pr|^2 - <Pr, mean_j Nr_j>)))
//   total  = L_bpr + L_rate + L_rank + L_iden
//
// The only coupling across records is L_iden's column mean: with c_b = beta wi / B (sigmoid(x_b) - z_b) every row of
// d gn receives the same vector G = -(1/B) sum_b c_b gp_b.
//
// Five plain launches on one stream (no atomics, every sum in an order fixed by B and d -> two identical calls give
// identical bits).  A workgroup is four waves and owns a chunk of ALDI_CHUNK = 16 consecutive records, four per wave, one
// record per wave at a time, lane l holding columns 4 l .. 4 l + 3 (16-byte loads):
//   mean part     column sums of gn and of the gathered Nr over the chunk -> one partial of 2 d floats per chunk;
//   mean finish   one workgroup adds the partials (wave g the chunks g, g + 4, ... in order, then (0 + 1) + (2 + 3)) -> the means;
//   record        the eight dot products, the coefficients, the three gradient rows (d gn without G) and the chunk's
//                 sum c_b gp_b and four loss sums -> one partial of d + 4 floats per chunk;
//   cross finish  one workgroup adds those partials in the same order -> G and loss5;
//   neg add       d gn += G, every row (skipped without d gn).
#include <math.h>

#include "loss_common.h"

namespace {

constexpr int ALDI_CHUNK = 16;          // records per workgroup: 4 waves x ALDI_PER_WAVE
constexpr int ALDI_PER_WAVE = 4;

// sigmoid(x), 1 - sigmoid(x) (formed without the subtraction) and log1p(exp(-|x|))
__device__ __forceinline__ void aldi_sigmoid(float x, float* s, float* one_minus, float* softplus_tail) {
    const float e = expf(-fabsf(x)), inv = 1.f / (1.f + e);
    *s = x >= 0.f ? inv : e * inv;
    *one_minus = x >= 0.f ? e * inv : inv;
    *softplus_tail = log1pf(e);
}

// bce(x, z) and sigmoid(x) - z for z = sigmoid(t): x - x z and the difference of two saturated sigmoids are taken from
// 1 - z = sigmoid(-t), which stays exact where z rounds to 1
__device__ __forceinline__ float aldi_bce(float x, float t, float* slope) {
    float s, oms, tail, z, omz, unused;
    aldi_sigmoid(x, &s, &oms, &tail);
    aldi_sigmoid(t, &z, &omz, &unused);
    *slope = (x >= 0.f && t >= 0.f) ? omz - oms : s - z;
    return (x >= 0.f ? x * omz : -x * z) + tail;
}

__device__ __forceinline__ float aldi_sign(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

// the four waves' values of one lane, added as (0 + 1) + (2 + 3); every thread of the workgroup calls it
__device__ __forceinline__ f32x4 aldi_block_sum(f32x4 v, f32x4 (*red)[64], int wave, int lane) {
    __syncthreads();                                   // (the previous use of red is over)
    red[wave][lane] = v;
    __syncthreads();
    return (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}

// column quad q of the chunks' partials: wave g adds the chunks g, g + 4, ... in order, then the four waves
__device__ __forceinline__ f32x4 aldi_chunk_sum(const float* __restrict__ part, int64_t n_chunks, int width, int q,
                                                f32x4 (*red)[64], int wave, int lane) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (4 * q < width)
        for (int64_t ch = wave; ch < n_chunks; ch += 4) acc += *reinterpret_cast<const f32x4*>(part + ch * width + 4 * q);
    return aldi_block_sum(acc, red, wave, lane);
}

// ---- mean part: one workgroup per chunk ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void aldi_mean_part_kernel(const float* __restrict__ vt, int64_t item_rows,
                                                             const int32_t* __restrict__ neg,
                                                             const float* __restrict__ gn, int64_t batch, int d,
                                                             float* __restrict__ part) {
    __shared__ f32x4 red[4][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, col = 4 * lane;
    const bool ok = col < d;
    const int64_t b0 = (int64_t)blockIdx.x * ALDI_CHUNK + wave * ALDI_PER_WAVE;
    f32x4 sg = {0.f, 0.f, 0.f, 0.f}, sv = sg;
#pragma unroll
    for (int j = 0; j < ALDI_PER_WAVE; ++j) {
        const int64_t b = b0 + j;
        if (b >= batch) break;
        const int64_t n = neg[b];
        sg += lg_load4(gn + b * d + col, ok);
        sv += lg_load4(vt + n * d + col, ok && n >= 0 && n < item_rows);
    }
    sg = aldi_block_sum(sg, red, wave, lane);
    sv = aldi_block_sum(sv, red, wave, lane);
    if (wave == 0 && ok) {
        float* p = part + (int64_t)blockIdx.x * 2 * d;
        *reinterpret_cast<f32x4*>(p + col) = sg;
        *reinterpret_cast<f32x4*>(p + d + col) = sv;
    }
}

// ---- mean finish: one workgroup --------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void aldi_mean_finish_kernel(const float* __restrict__ part, int64_t n_chunks, int d,
                                                               float inv_b, float* __restrict__ mean) {
    __shared__ f32x4 red[4][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, width = 2 * d;
    for (int q0 = 0; 4 * q0 < width; q0 += 64) {
        const int q = q0 + lane;
        const f32x4 s = aldi_chunk_sum(part, n_chunks, width, q, red, wave, lane);
        if (wave == 0 && 4 * q < width) *reinterpret_cast<f32x4*>(mean + 4 * q) = s * inv_b;
    }
}

// ---- record: one workgroup per chunk, one wave per record at a time --------------------------------------------------
// part[chunk] = d + 4 floats: sum c_b gp_b (times the scale), then the sums of the four per-record loss terms
__global__ __launch_bounds__(256) void aldi_record_kernel(
    const float* __restrict__ ut, int64_t user_rows, const float* __restrict__ vt, int64_t item_rows,
    const int32_t* __restrict__ users, const int32_t* __restrict__ pos, const int32_t* __restrict__ neg,
    const float* __restrict__ gu, const float* __restrict__ gp, const float* __restrict__ gn, const float* __restrict__ w,
    const float* __restrict__ mean, int64_t batch, int d, float inv_b, float alpha_b, float beta_b, float gamma_b,
    float scale, float* __restrict__ dgu, float* __restrict__ dgp, float* __restrict__ dgn, float* __restrict__ part) {
    __shared__ f32x4 red[4][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, col = 4 * lane;
    const bool ok = col < d;
    const int64_t b0 = (int64_t)blockIdx.x * ALDI_CHUNK + wave * ALDI_PER_WAVE;
    const f32x4 mg = lg_load4(mean + col, ok), mv = lg_load4(mean + d + col, ok);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f}, terms = acc;
#pragma unroll 1
    for (int j = 0; j < ALDI_PER_WAVE; ++j) {
        const int64_t b = b0 + j;
        if (b >= batch) break;
        const int64_t u = users[b], p = pos[b], n = neg[b], o = b * d + col;
        // (uniform: a record whose ids leave the tables contributes nothing instead of reading wild)
        const bool in = u >= 0 && u < user_rows && p >= 0 && p < item_rows && n >= 0 && n < item_rows;
        const bool on = ok && in;
        const f32x4 ur = lg_load4(ut + u * d + col, on), pr = lg_load4(vt + p * d + col, on);
        const f32x4 nr = lg_load4(vt + n * d + col, on);
        const f32x4 xu = lg_load4(gu + o, on), xp = lg_load4(gp + o, on), xn = lg_load4(gn + o, on);
        const float wi = in ? w[p] : 0.f;
        const float sp = lg_wave_sum(lg_dot4(xu, xp)), sn = lg_wave_sum(lg_dot4(xu, xn));
        const float tp = lg_wave_sum(lg_dot4(ur, pr)), tn = lg_wave_sum(lg_dot4(ur, nr));
        const float pp = lg_wave_sum(lg_dot4(xp, xp)), pm = lg_wave_sum(lg_dot4(xp, mg));
        const float tpp = lg_wave_sum(lg_dot4(pr, pr)), tpm = lg_wave_sum(lg_dot4(pr, mv));

        const float x = sp - sn;
        float s, oms, tail;
        aldi_sigmoid(x, &s, &oms, &tail);
        const float l_bpr = -logf(1e-5f + s), d_bpr = -s * oms / (1e-5f + s);
        const float r1 = tp - sp, r2 = tn - sn;
        float k_rank, k_iden;
        const float l_rank = wi * aldi_bce(x, tp - tn, &k_rank);
        const float l_iden = wi * aldi_bce(pp - pm, tpp - tpm, &k_iden);
        const float a_x = inv_b * d_bpr + alpha_b * wi * k_rank;
        const float a_p = in ? scale * (a_x - gamma_b * aldi_sign(r1)) : 0.f;
        const float a_n = in ? scale * (-a_x - gamma_b * aldi_sign(r2)) : 0.f;
        const float c = scale * beta_b * wi * k_iden;
        if (ok) {
            if (dgu) *reinterpret_cast<f32x4*>(dgu + o) = xp * a_p + xn * a_n;
            if (dgp) *reinterpret_cast<f32x4*>(dgp + o) = xu * a_p + (xp * 2.f - mg) * c;
            if (dgn) *reinterpret_cast<f32x4*>(dgn + o) = xu * a_n;
        }
        acc += xp * c;
        if (in) terms += f32x4{l_bpr, fabsf(r1) + fabsf(r2), l_rank, l_iden};
    }
    acc = aldi_block_sum(acc, red, wave, lane);
    terms = aldi_block_sum(terms, red, wave, lane);
    if (wave == 0) {
        float* p = part + (int64_t)blockIdx.x * (d + 4);
        if (ok) *reinterpret_cast<f32x4*>(p + col) = acc;
        if (lane == 0) *reinterpret_cast<f32x4*>(p + d) = terms;
    }
}

// ---- cross finish: one workgroup -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void aldi_cross_finish_kernel(const float* __restrict__ part, int64_t n_chunks, int d,
                                                                float inv_b, float alpha, float beta, float gamma,
                                                                float* __restrict__ gvec, float* __restrict__ loss) {
    __shared__ f32x4 red[4][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, width = d + 4, last = d / 4;
    for (int q0 = 0; 4 * q0 < width; q0 += 64) {
        const int q = q0 + lane;
        const f32x4 s = aldi_chunk_sum(part, n_chunks, width, q, red, wave, lane);
        if (wave != 0) continue;
        if (q < last) *reinterpret_cast<f32x4*>(gvec + 4 * q) = s * -inv_b;
        if (q == last && loss) {
            const float l0 = s[0] * inv_b, l1 = gamma * (s[1] * inv_b), l2 = alpha * (s[2] * inv_b);
            const float l3 = beta * (s[3] * inv_b);
            loss[0] = l0, loss[1] = l1, loss[2] = l2, loss[3] = l3;
            loss[4] = (l0 + l1) + (l2 + l3);
        }
    }
}

// ---- neg add: d gn += G ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void aldi_neg_add_kernel(const float* __restrict__ gvec, int64_t batch, int d,
                                                           float* __restrict__ dgn) {
    const int per_row = d / 4;
    const int64_t total = batch * per_row;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int col = 4 * (int)(i % per_row);
        f32x4* p = reinterpret_cast<f32x4*>(dgn) + i;
        *p += *reinterpret_cast<const f32x4*>(gvec + col);
    }
}

struct AldiWs {
    float *mean_part, *mean, *part, *gvec;
    size_t bytes;
};

int64_t aldi_chunks(int64_t batch) { return (batch + ALDI_CHUNK - 1) / ALDI_CHUNK; }

bool aldi_shape_ok(int64_t batch, int d) {
    return batch >= 1 && batch < ((int64_t)1 << 31) && lg_width_ok(d);
}

AldiWs aldi_layout(void* base, int64_t batch, int d) {
    const int64_t n = aldi_chunks(batch);
    AldiWs w;
    WsCarver c(base);
    w.mean_part = c.take(n * 2 * d);
    w.mean = c.take(2 * d);
    w.part = c.take(n * (d + 4));
    w.gvec = c.take(d);
    w.bytes = c.bytes;
    return w;
}

}  // namespace

extern "C" size_t crh_aldi_workspace_bytes(int64_t batch, int d) {
    if (!aldi_shape_ok(batch, d)) return 0;
    return aldi_layout(nullptr, batch, d).bytes;
}

extern "C" int crh_aldi_f32(const float* user_table, int64_t user_rows, const float* item_table, int64_t item_rows,
                            const int32_t* users, const int32_t* pos, const int32_t* neg, int user_min, int user_max,
                            int item_min, int item_max, const float* gen_user, const float* gen_pos, const float* gen_neg,
                            const float* item_weight, int64_t batch, int d, float alpha, float beta, float gamma,
                            float scale, float* grad_user, float* grad_pos, float* grad_neg, float* loss_out,
                            void* workspace, size_t workspace_bytes, void* stream) {
    CRH_CHECK_ARG(user_table && item_table && item_weight, "crh_aldi_f32: NULL table pointer");
    CRH_CHECK_ARG(users && pos && neg, "crh_aldi_f32: NULL id pointer");
    CRH_CHECK_ARG(gen_user && gen_pos && gen_neg, "crh_aldi_f32: NULL tower output pointer");
    CRH_CHECK_ARG(grad_user || grad_pos || grad_neg || loss_out, "crh_aldi_f32: NULL gradients and loss: nothing to compute");
    LG_CHECK_WIDTH("crh_aldi_f32", d);
    CRH_CHECK_ARG(batch >= 1 && batch < ((int64_t)1 << 31), "crh_aldi_f32: batch = %lld must lie in [1, 2^31)",
                  (long long)batch);
    LG_CHECK_IDS("crh_aldi_f32", "user", user_min, user_max, user_rows);
    LG_CHECK_IDS("crh_aldi_f32", "item", item_min, item_max, item_rows);
    CRH_CHECK_ARG(isfinite(alpha) && isfinite(beta) && isfinite(gamma) && isfinite(scale),
                  "crh_aldi_f32: alpha, beta, gamma and scale must be finite");
    CRH_CHECK_ARG(lg_aligned16(user_table, item_table, gen_user, gen_pos, gen_neg, grad_user, grad_pos, grad_neg),
                  "crh_aldi_f32: tables, tower outputs and gradients must be 16-byte aligned");
    LG_CHECK_WS("crh_aldi_f32", workspace, workspace_bytes, crh_aldi_workspace_bytes(batch, d));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const AldiWs w = aldi_layout(workspace, batch, d);
    const int64_t n_chunks = aldi_chunks(batch);
    const float inv_b = 1.f / (float)batch;
    hipLaunchKernelGGL(aldi_mean_part_kernel, dim3((unsigned)n_chunks), dim3(256), 0, st, item_table, item_rows, neg, gen_neg,
                       batch, d, w.mean_part);
    hipLaunchKernelGGL(aldi_mean_finish_kernel, dim3(1), dim3(256), 0, st, w.mean_part, n_chunks, d, inv_b, w.mean);
    hipLaunchKernelGGL(aldi_record_kernel, dim3((unsigned)n_chunks), dim3(256), 0, st, user_table, user_rows, item_table,
                       item_rows, users, pos, neg, gen_user, gen_pos, gen_neg, item_weight, w.mean, batch, d, inv_b,
                       alpha * inv_b, beta * inv_b, gamma * inv_b, scale, grad_user, grad_pos, grad_neg, w.part);
    hipLaunchKernelGGL(aldi_cross_finish_kernel, dim3(1), dim3(256), 0, st, w.part, n_chunks, d, inv_b, alpha, beta, gamma,
                       w.gvec, loss_out);
    if (grad_neg) {
        const int64_t blocks = (batch * (d / 4) + 255) / 256;
        hipLaunchKernelGGL(aldi_neg_add_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st, w.gvec,
                           batch, d, grad_neg);
    }
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}
