// The optimisers of the training path for gfx950: torch.optim.Adam and plain torch.optim.SGD, dense and touched-rows.
//
// What is in this file:
//   * adam_dense_kernel (crh_adam_dense_f32): torch/optim/adam.py _single_tensor_adam with default flags, op for op
//     (adam_elem4 in crh_common.h) -- EVERY element of both tables moves every step -- and the gradient
//     is zeroed in the same pass;
//   * sgd_dense_kernel (crh_sgd_dense_f32): p <- fma(-lr, g, p);
//   * adam_rows_kernel (crh_adam_rows_f32): the touched-rows replay of dense Adam, bit for bit the dense result;
//   * sgd_rows_kernel (crh_sgd_rows_f32): SGD on the rows of one batch's plan (bpr_plan.h);
//   * the step-dependent Adam factors, derived on the host in one place (adam_step_scalars) for
//     crh_adam_step_scalars_host, crh_adam_step_scalars_range_host and crh_adam_dense_f32.
// All of it is HBM-bound streaming with 16 B per lane.
#include <math.h>

#include "bpr_plan.h"
#include "train_common.h"

namespace {

// ---------------------------------------------------------------- dense Adam (+ zero the gradient)
struct AdamSeg {
    float* p;
    float* g;
    float* m;
    float* v;
    int64_t n4;   // elements / 4
};

__global__ __launch_bounds__(256) void adam_dense_kernel(AdamSeg s0, AdamSeg s1, float one_minus_b1, float b2,
                                                         float one_minus_b2, float bc2_sqrt, float eps,
                                                         float neg_step_size, int zero_grad,
                                                         const float* __restrict__ step_scalars) {
    if (step_scalars) {   // step-dependent factors from memory: lets a captured hipGraph be replayed every epoch
        bc2_sqrt = step_scalars[0];
        neg_step_size = step_scalars[1];
    }
    const int64_t total = s0.n4 + s1.n4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const bool first = i < s0.n4;
        const AdamSeg& s = first ? s0 : s1;
        const int64_t j = first ? i : i - s0.n4;
        f32x4* P = reinterpret_cast<f32x4*>(s.p) + j;
        f32x4* G = reinterpret_cast<f32x4*>(s.g) + j;
        f32x4* M = reinterpret_cast<f32x4*>(s.m) + j;
        f32x4* V = reinterpret_cast<f32x4*>(s.v) + j;
        const AdamK k{one_minus_b1, b2, one_minus_b2, eps};
        if (zero_grad & 2) {   // streaming tables (far beyond the caches): nontemporal accesses
            f32x4 p = __builtin_nontemporal_load(P), g = __builtin_nontemporal_load(G);
            f32x4 m = __builtin_nontemporal_load(M), v = __builtin_nontemporal_load(V);
            adam_elem4(p, m, v, g, k, bc2_sqrt, neg_step_size);
            __builtin_nontemporal_store(p, P);
            __builtin_nontemporal_store(m, M);
            __builtin_nontemporal_store(v, V);
            if (zero_grad & 1) __builtin_nontemporal_store(f32x4{0.f, 0.f, 0.f, 0.f}, G);
            continue;
        }
        f32x4 p = *P, g = *G, m = *M, v = *V;
        adam_elem4(p, m, v, g, k, bc2_sqrt, neg_step_size);
        *P = p; *M = m; *V = v;
        if (zero_grad) *G = f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// ---------------------------------------------------------------- plain SGD (north_star's "BPR loss + SGD update")
// torch.optim.SGD defaults (no momentum, no weight decay): p <- p + (-lr) * g, ONE fused multiply-add per element
// (the canonical form of this build: oracle/oracle_np.py sgd_dense; ATen's vectorised add_(g, alpha=-lr) uses
// an fma as well).  SURVEY.md F3: the reference trains with Adam, SGD is the extra mode the north_star names.
// A row whose gradient is zero does not move, so the dense pass and the touched-rows pass give the same tables.
__global__ __launch_bounds__(256) void sgd_dense_kernel(float* __restrict__ p, float* __restrict__ g, int64_t n4,
                                                        float neg_lr, int zero_grad) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        f32x4* P = reinterpret_cast<f32x4*>(p) + i;
        f32x4* G = reinterpret_cast<f32x4*>(g) + i;
        f32x4 x = *P;
        sgd_elem4(x, *G, neg_lr);
        *P = x;
        if (zero_grad) *G = f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// ---------------------------------------------------------------- touched-rows replay of dense Adam
// torch.optim.Adam moves EVERY row every step: a row whose gradient is zero still decays its
// moments and drifts by its stale momentum.  At catalogue scale (S-TRAIN-XL: 11 M rows, 196 K touched per
// step) the dense pass is 99.5 % of the step's HBM traffic.  But rows are independent and the update is
// elementwise, so a row that is not touched between steps s and t can be brought up to date LATER by
// replaying its zero-gradient steps s+1..t-1 in registers -- the same fp32 operations in the same order,
// hence the same bits as the dense kernel -- provided the step-dependent factors of every step are at hand
// (`table`: [step][2] = {sqrt(1-beta2^step), -lr/(1-beta1^step)}, step 1 at index 1).  `last[row]` is the
// step the row's (p, m, v) are valid for.
//   mode 0  catch-up  rows of the plan -> valid for step `step` - 1      (before the forward pass of `step`)
//   mode 1  step      rows of the plan: apply step `step` with g = G[row], clear G[row]
//   mode 2  flush     ALL rows -> valid for step `step`                   (before the tables are read)
struct AdamRowsArgs {
    float *p, *g, *m, *v;
    int32_t* last;
    int64_t n_rows;        // rows of the table (mode 2)
    int d;
    const int32_t* plan;   // modes 0/1: touched rows (users, then items offset by user_rows)
    int64_t user_rows;
    int64_t step;
    const float* table;
    AdamK k;
    int mode;
};

template <int G>
__global__ __launch_bounds__(256) void adam_rows_kernel(AdamRowsArgs a) {
    const int lig = threadIdx.x % G;
    const int64_t gid = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    const int64_t gstride = (int64_t)gridDim.x * (256 / G);
    const int nvec = a.d >> 2;
    int64_t n_work = a.n_rows;
    PlanView pv{};
    if (a.mode != 2) {
        pv = plan_view(a.plan);
        n_work = (int64_t)pv.n_u + pv.n_i;
    }
    for (int64_t w = gid; w < n_work; w += gstride) {
        int64_t row = w;
        if (a.mode != 2) row = w < pv.n_u ? (int64_t)pv.urow[w] : a.user_rows + pv.irow[w - pv.n_u];
        const int64_t from = (int64_t)a.last[row] + 1;
        const int64_t upto = a.mode == 0 ? a.step - 1 : (a.mode == 1 ? a.step - 1 : a.step);   // zero-gradient part
        if (a.mode != 1 && from > upto) continue;
        for (int c = lig; c < nvec; c += G) {
            const int64_t o = row * a.d + (int64_t)c * 4;
            f32x4 p = *reinterpret_cast<f32x4*>(a.p + o);
            f32x4 m = *reinterpret_cast<f32x4*>(a.m + o);
            f32x4 v = *reinterpret_cast<f32x4*>(a.v + o);
            for (int64_t s = from; s <= upto; ++s) {
                const float bc2_sqrt = a.table[2 * s], nss = a.table[2 * s + 1];
                adam_elem4(p, m, v, f32x4{0.f, 0.f, 0.f, 0.f}, a.k, bc2_sqrt, nss);
            }
            if (a.mode == 1) {
                const f32x4 g = *reinterpret_cast<f32x4*>(a.g + o);
                const float bc2_sqrt = a.table[2 * a.step], nss = a.table[2 * a.step + 1];
                adam_elem4(p, m, v, g, a.k, bc2_sqrt, nss);
                *reinterpret_cast<f32x4*>(a.g + o) = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            *reinterpret_cast<f32x4*>(a.p + o) = p;
            *reinterpret_cast<f32x4*>(a.m + o) = m;
            *reinterpret_cast<f32x4*>(a.v + o) = v;
        }
        // all lanes of the group have read last[row] before anyone overwrites it (same wave, in order)
        if (lig == 0) a.last[row] = (int32_t)(a.mode == 0 ? a.step - 1 : a.step);
    }
}

// SGD on the rows of a batch's plan only (users, then items offset by user_rows): p[row] += -lr * g[row], g[row] = 0.
// Equal to sgd_dense_kernel over the whole table (untouched rows have a zero gradient), at 3 x 16 B per touched
// element instead of a pass over every row: the update of choice at catalogue scale.
template <int G>
__global__ __launch_bounds__(256) void sgd_rows_kernel(float* __restrict__ p, float* __restrict__ g, int d,
                                                       const int32_t* __restrict__ plan, int64_t user_rows,
                                                       float neg_lr) {
    const PlanView pv = plan_view(plan);
    const int lig = threadIdx.x % G;
    const int nvec = d >> 2;
    const int64_t n_work = (int64_t)pv.n_u + pv.n_i;
    for (int64_t w = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G; w < n_work; w += (int64_t)gridDim.x * (256 / G)) {
        const int64_t row = w < pv.n_u ? (int64_t)pv.urow[w] : user_rows + pv.irow[w - pv.n_u];
        for (int c = lig; c < nvec; c += G) {
            const int64_t o = row * d + (int64_t)c * 4;
            f32x4 x = *reinterpret_cast<f32x4*>(p + o);
            sgd_elem4(x, *reinterpret_cast<const f32x4*>(g + o), neg_lr);
            *reinterpret_cast<f32x4*>(p + o) = x;
            *reinterpret_cast<f32x4*>(g + o) = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
}

// The two step-dependent Adam factors {sqrt(1-beta2^step), -lr/(1-beta1^step)}: in double like torch (python floats),
// then cast.  The one place they are derived.
void adam_step_scalars(double lr, double beta1, double beta2, int64_t step, float* out2) {
    const double bc1 = 1.0 - pow(beta1, (double)step);
    const double bc2 = 1.0 - pow(beta2, (double)step);
    out2[0] = (float)sqrt(bc2);
    out2[1] = (float)(-(lr / bc1));
}

}  // namespace

extern "C" int crh_adam_dense_f32(float* p0, float* g0, float* m0, float* v0, int64_t n0, float* p1, float* g1,
                                  float* m1, float* v1, int64_t n1, double lr, double beta1, double beta2,
                                  double eps, int64_t step, int zero_grad, const float* step_scalars,
                                  void* stream) {
    CRH_CHECK_ARG(p0 && g0 && m0 && v0 && n0 > 0, "crh_adam_dense_f32: NULL / empty first tensor");
    CRH_CHECK_ARG(n1 == 0 || (p1 && g1 && m1 && v1), "crh_adam_dense_f32: NULL second tensor");
    CRH_CHECK_ARG(n0 % 4 == 0 && n1 % 4 == 0, "crh_adam_dense_f32: element counts must be multiples of 4");
    CRH_CHECK_ARG(step >= 1 || step_scalars, "crh_adam_dense_f32: step starts at 1");
    if (step < 1) step = 1;
    float sc[2];
    adam_step_scalars(lr, beta1, beta2, step, sc);
    AdamSeg s0{p0, g0, m0, v0, n0 / 4}, s1{p1, g1, m1, v1, n1 / 4};
    const int64_t total = s0.n4 + s1.n4;
    int64_t blocks = (total + 255) / 256;
    // measured at S-TRAIN-XL (45 GB per launch): 2048 blocks 8.73 ms, 16384 blocks + nontemporal accesses 8.03 ms
    // (HISTORY.md section 5, round 1); tables beyond 256 MB stream with nontemporal accesses
    if (blocks > 16384) blocks = 16384;
    const int zg = (zero_grad ? 1 : 0) | (total * 16 > ((int64_t)256 << 20) ? 2 : 0);
    hipLaunchKernelGGL(adam_dense_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       s0, s1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), sc[0], (float)eps, sc[1], zg,
                       step_scalars);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

// torch.optim.SGD(lr) defaults on a dense tensor: p <- fma(-lr, g, p); zero_grad != 0 also clears g.
extern "C" int crh_sgd_dense_f32(float* p, float* g, int64_t n, double lr, int zero_grad, void* stream) {
    CRH_CHECK_ARG(p && g && n > 0 && n % 4 == 0, "crh_sgd_dense_f32: NULL tensor / element count not a multiple of 4");
    CRH_CHECK_ARG((((uintptr_t)p | (uintptr_t)g) & 15) == 0, "crh_sgd_dense_f32: tensors must be 16-byte aligned");
    int64_t blocks = (n / 4 + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(sgd_dense_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p, g,
                       n / 4, (float)(-lr), zero_grad);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

// The same update on the rows of one batch's plan only (bit-identical tables: a zero gradient moves nothing);
// clears the gradient rows it consumed.  p, g: (n_rows, d) tables, users first, item rows offset by user_rows.
extern "C" int crh_sgd_rows_f32(float* p, float* g, int d, const int32_t* plan, int64_t batch, int64_t user_rows,
                                double lr, void* stream) {
    CRH_CHECK_ARG(p && g && plan && batch > 0, "crh_sgd_rows_f32: NULL pointer / empty batch");
    CRH_CHECK_ARG(d >= 4 && d % 4 == 0, "crh_sgd_rows_f32: d=%d must be a positive multiple of 4", d);
    const int G = pick_group(d);
    int64_t blocks = (3 * batch + (256 / G) - 1) / (256 / G);
    if (blocks > 8192) blocks = 8192;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dispatch_group(G, [&](auto gc) -> int {
        constexpr int GG = decltype(gc)::value;
        hipLaunchKernelGGL(sgd_rows_kernel<GG>, dim3((unsigned)blocks), dim3(256), 0, st, p, g, d, plan, user_rows,
                           (float)(-lr));
        CRH_HIP(hipGetLastError());
        return CRH_OK;
    });
}

// Touched-rows replay of dense Adam (see adam_rows_kernel).  p, g, m, v: (n_rows, d) fp32 tables, users first;
// last_step (n_rows) int32, all zero at the start (every row valid for "step 0"); plan: a batch's reverse index
// (crh_bpr_plan_build*), its item rows are offset by user_rows; scalar_table: device floats [2*(max_step+1)],
// entry s = {sqrt(1-beta2^s), -lr/(1-beta1^s)} (crh_adam_step_scalars_host); mode 0/1/2 = catch-up / step /
// flush.  Interleaving  catch-up(t) -> forward/backward(t) -> step(t)  for t = 1, 2, ... and a flush(T)
// before the tables are read reproduces crh_adam_dense_f32 applied T times bit for bit.
extern "C" int crh_adam_rows_f32(float* p, float* g, float* m, float* v, int32_t* last_step, int64_t n_rows, int d,
                                 const int32_t* plan, int64_t batch, int64_t user_rows, int64_t step,
                                 const float* scalar_table, double beta1, double beta2, double eps, int mode,
                                 void* stream) {
    CRH_CHECK_ARG(p && m && v && last_step && scalar_table && n_rows > 0, "crh_adam_rows_f32: NULL / empty table");
    CRH_CHECK_ARG(d >= 4 && d % 4 == 0, "crh_adam_rows_f32: d=%d must be a positive multiple of 4", d);
    CRH_CHECK_ARG(mode >= 0 && mode <= 2, "crh_adam_rows_f32: mode %d outside 0..2", mode);
    CRH_CHECK_ARG(mode == 2 || (plan && batch > 0), "crh_adam_rows_f32: modes 0/1 need the batch's plan");
    CRH_CHECK_ARG(mode != 1 || g, "crh_adam_rows_f32: mode 1 needs the gradient table");
    CRH_CHECK_ARG(step >= (mode == 2 ? 0 : 1), "crh_adam_rows_f32: step starts at 1");
    AdamRowsArgs a{p, g, m, v, last_step, n_rows, d, plan, user_rows, step, scalar_table,
                   AdamK{(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps}, mode};
    const int G = pick_group(d);
    const int64_t work = mode == 2 ? n_rows : 3 * batch;
    int64_t blocks = (work + (256 / G) - 1) / (256 / G);
    if (blocks > 8192) blocks = 8192;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dispatch_group(G, [&](auto gc) -> int {
        constexpr int GG = decltype(gc)::value;
        hipLaunchKernelGGL(adam_rows_kernel<GG>, dim3((unsigned)blocks), dim3(256), 0, st, a);
        CRH_HIP(hipGetLastError());
        return CRH_OK;
    });
}

// HOST helpers for callers that keep the step-dependent Adam factors in device memory (graph replay, the touched-rows
// table): the pair of one step, exactly as crh_adam_dense_f32 derives it ...
extern "C" void crh_adam_step_scalars_host(double lr, double beta1, double beta2, int64_t step, float* out2_host) {
    adam_step_scalars(lr, beta1, beta2, step, out2_host);
}

// ... and of steps first_step .. first_step + n - 1 (out: n pairs).
extern "C" void crh_adam_step_scalars_range_host(double lr, double beta1, double beta2, int64_t first_step, int64_t n,
                                                 float* out_host) {
    for (int64_t i = 0; i < n; ++i) adam_step_scalars(lr, beta1, beta2, first_step + i, out_host + 2 * i);
}
