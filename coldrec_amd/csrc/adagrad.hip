// torch.optim.Adagrad's defaults (lr_decay = 0, weight_decay = 0, initial accumulator 0) over the rows a batch touched:
// for each of the n_ids distinct rows, element by element and every operation rounded on its own, as the separate ATen
// ops of torch/optim/adagrad.py _single_tensor_adagrad do:
//
//   s <- s + g * g                      state_sum.addcmul_(grad, grad, value=1)
//   std = sqrt(s) + eps                 state_sum.sqrt().add_(eps)
//   p <- p + (-lr) * (g / std)          param.addcdiv_(grad, std, value=-clr), clr = lr
//
// then the consumed gradient row is cleared (zero_grad).  A zero gradient leaves s and p with their bits (s + 0, p + -0),
// so the pass over the touched rows equals the dense step.  One lane group per row, four columns per lane.
#include <math.h>

#include "loss_common.h"

namespace {

__device__ __forceinline__ void adagrad_elem4(f32x4& p, f32x4& s, const f32x4& g, float neg_lr, float eps) {
#pragma clang fp contract(off)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float sc = s[c] + g[c] * g[c];
        const float sd = sqrtf(sc) + eps;
        p[c] = p[c] + neg_lr * (g[c] / sd);
        s[c] = sc;
    }
}

template <int LPR>
__global__ __launch_bounds__(64) void adagrad_rows_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ s,
                                                          const int32_t* __restrict__ ids, int64_t n_ids, int64_t n_rows,
                                                          int d, float neg_lr, float eps, int zero_grad) {
    constexpr int RG = 64 / LPR;
    const auto [lane, cl, grp, col] = lg_coords<LPR>();
    const int64_t k = (int64_t)blockIdx.x * RG + grp;
    if (k >= n_ids || col >= d) return;
    const int64_t id = ids[k];
    if (id < 0 || id >= n_rows) return;                 // (an id outside the table updates nothing instead of writing wild)
    const int64_t o = id * d + col;
    const f32x4 gv = *reinterpret_cast<const f32x4*>(g + o);
    f32x4 sv = *reinterpret_cast<const f32x4*>(s + o), pv = *reinterpret_cast<const f32x4*>(p + o);
    adagrad_elem4(pv, sv, gv, neg_lr, eps);
    *reinterpret_cast<f32x4*>(s + o) = sv;
    *reinterpret_cast<f32x4*>(p + o) = pv;
    if (zero_grad) *reinterpret_cast<f32x4*>(g + o) = f32x4{0.f, 0.f, 0.f, 0.f};
}

}  // namespace

extern "C" int crh_adagrad_rows_f32(float* p, float* g, float* state_sum, const int32_t* ids, int64_t n_ids, int64_t n_rows,
                                    int d, double lr, double eps, int zero_grad, void* stream) {
    CRH_CHECK_ARG(p && g && state_sum && ids, "crh_adagrad_rows_f32: NULL p, g, state_sum or ids pointer");
    LG_CHECK_WIDTH("crh_adagrad_rows_f32", d);
    CRH_CHECK_ARG(n_ids >= 0 && n_ids <= n_rows && n_rows < ((int64_t)1 << 31),
                  "crh_adagrad_rows_f32: n_ids = %lld out of [0, n_rows = %lld], n_rows < 2^31", (long long)n_ids,
                  (long long)n_rows);
    CRH_CHECK_ARG(isfinite(lr) && isfinite(eps) && eps >= 0., "crh_adagrad_rows_f32: lr and eps must be finite, eps >= 0");
    CRH_CHECK_ARG(lg_aligned16(p, g, state_sum), "crh_adagrad_rows_f32: p, g and state_sum must be 16-byte aligned");
    CRH_CHECK_ARG(p != g && p != state_sum && g != state_sum, "crh_adagrad_rows_f32: p, g and state_sum must not alias");
    if (n_ids == 0) return CRH_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    lg_dispatch_lpr(d, [&](auto lpr) {
        constexpr int LPR = decltype(lpr)::value, RG = 64 / LPR;
        hipLaunchKernelGGL((adagrad_rows_kernel<LPR>), dim3((unsigned)((n_ids + RG - 1) / RG)), dim3(64), 0, st, p, g, state_sum,
                           ids, n_ids, n_rows, d, (float)-lr, (float)eps, zero_grad);
    });
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}
