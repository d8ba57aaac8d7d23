// The loss of DeepMusic (reference model/DeepMusic.py:19-29, util/utils.py:32-48), forward and backward in one call.  One
// frozen table T (rows, d), B ids into it, B generated rows G (B, d), one per record:
//
//   L_mse = sum |T[id_b] - G_b|^2 / (B d)        R = reg |G|_F / B        total = L_mse + R
//   d total / d G_b = 2 (G_b - T[id_b]) / (B d) + reg G_b / (B |G|_F)     (second part 0 when |G|_F = 0, as torch's norm
//                                                                          backward has it)
//
// The only coupling across records is R's norm.  The table is frozen: no gradient, no owner pass.
//
// Three plain launches on one stream, gar.hip's sequence (no atomics, every sum in an order fixed by B and d -> two
// identical calls give identical bits).  A lane group of LPR = pow2(d / 4) lanes holds one row, four columns per lane:
//   record   one lane group per record: the two sums of squares and grad_gen's row without R's part;
//   loss     one workgroup adds the B records' terms in index order -> loss_out and the factor reg / (B |G|_F);
//   gen      grad_gen += factor G, every row (skipped without grad_gen).
#include <math.h>

#include "loss_common.h"

namespace {

// ---- record: one lane group per record ------------------------------------------------------------------------------
// rec[b] = |T[id_b] - G_b|^2, |G_b|^2, 0, 0;  wm = scale 2 / (B d)
template <int LPR>
__global__ __launch_bounds__(64) void deepmusic_record_kernel(const float* __restrict__ table, int64_t rows,
                                                              const int32_t* __restrict__ ids,
                                                              const float* __restrict__ gen, int64_t batch, int d,
                                                              float wm, float* __restrict__ grad_gen,
                                                              float* __restrict__ rec) {
    constexpr int RG = 64 / LPR;
    const auto [lane, cl, grp, col] = lg_coords<LPR>();
    const int64_t b = (int64_t)blockIdx.x * RG + grp;
    const bool live = b < batch, ok = col < d;
    const int64_t id = live ? ids[b] : 0, at = b * d + col;
    // (a record whose id leaves the table contributes nothing instead of reading wild)
    const bool in = live && id >= 0 && id < rows, on = ok && in;
    const f32x4 tr = lg_load4(table + id * d + col, on), g = lg_load4(gen + at, on);
    const f32x4 df = g - tr;
    const float ssd = lg_group_sum<LPR>(lg_dot4(df, df)), ssg = lg_group_sum<LPR>(lg_dot4(g, g));
    if (live && ok && grad_gen) *reinterpret_cast<f32x4*>(grad_gen + at) = df * wm;
    if (live && cl == 0) *reinterpret_cast<f32x4*>(rec + b * 4) = f32x4{ssd, ssg, 0.f, 0.f};
}

// ---- loss: one workgroup --------------------------------------------------------------------------------------------
// rinv = scale reg / (B |G|_F) (0 for a zero norm)
__global__ __launch_bounds__(256) void deepmusic_loss_kernel(const float* __restrict__ rec, int64_t batch, int d, float reg,
                                                             float scale, float* __restrict__ loss,
                                                             float* __restrict__ rinv) {
    __shared__ float red[4][4];
    lg_record_sums(rec, batch, red);
    if (threadIdx.x == 0) {
        const float inv_b = 1.f / (float)batch;
        const float ssd = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
        const float ssg = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
        const float nrm = sqrtf(ssg);
        rinv[0] = ssg > 0.f ? scale * reg * inv_b / nrm : 0.f;
        if (loss) {
            const float l_mse = ssd * inv_b / (float)d, r = reg * nrm * inv_b;
            loss[0] = l_mse;
            loss[1] = r;
            loss[2] = l_mse + r;
        }
    }
}

// ---- gen: grad_gen += rinv[0] G -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void deepmusic_gen_add_kernel(const float* __restrict__ gen,
                                                                const float* __restrict__ rinv, int64_t quads,
                                                                float* __restrict__ grad_gen) {
    const float r = rinv[0];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < quads; i += (int64_t)gridDim.x * 256) {
        f32x4* p = reinterpret_cast<f32x4*>(grad_gen) + i;
        *p += reinterpret_cast<const f32x4*>(gen)[i] * r;
    }
}

struct DeepMusicWs {
    float *rec, *rinv;
    size_t bytes;
};

DeepMusicWs deepmusic_layout(void* base, int64_t batch) {
    DeepMusicWs w;
    WsCarver c(base);
    w.rec = c.take(batch * 4);
    w.rinv = c.take(4);
    w.bytes = c.bytes;
    return w;
}

bool deepmusic_shape_ok(int64_t batch, int d) { return batch >= 1 && batch < ((int64_t)1 << 31) && lg_width_ok(d); }

}  // namespace

extern "C" size_t crh_deepmusic_workspace_bytes(int64_t batch, int d) {
    if (!deepmusic_shape_ok(batch, d)) return 0;
    return deepmusic_layout(nullptr, batch).bytes;
}

extern "C" int crh_deepmusic_f32(const float* table, int64_t rows, const int32_t* ids, int id_min, int id_max,
                                 const float* gen, int64_t batch, int d, float reg, float scale, float* grad_gen,
                                 float* loss_out, void* workspace, size_t workspace_bytes, void* stream) {
    CRH_CHECK_ARG(table && gen, "crh_deepmusic_f32: NULL table pointer");
    CRH_CHECK_ARG(ids, "crh_deepmusic_f32: NULL id pointer");
    CRH_CHECK_ARG(grad_gen || loss_out, "crh_deepmusic_f32: NULL gradient and loss: nothing to compute");
    LG_CHECK_WIDTH("crh_deepmusic_f32", d);
    CRH_CHECK_ARG(batch >= 1 && batch < ((int64_t)1 << 31), "crh_deepmusic_f32: batch = %lld must lie in [1, 2^31)",
                  (long long)batch);
    LG_CHECK_IDS("crh_deepmusic_f32", "frozen", id_min, id_max, rows);
    CRH_CHECK_ARG(isfinite(reg) && isfinite(scale), "crh_deepmusic_f32: reg and scale must be finite");
    CRH_CHECK_ARG(lg_aligned16(table, gen, grad_gen),
                  "crh_deepmusic_f32: table, generated rows and gradient must be 16-byte aligned");
    LG_CHECK_WS("crh_deepmusic_f32", workspace, workspace_bytes, crh_deepmusic_workspace_bytes(batch, d));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const DeepMusicWs w = deepmusic_layout(workspace, batch);
    const float wm = scale * 2.f / (float)batch / (float)d;
    lg_dispatch_lpr(d, [&](auto lpr) {
        constexpr int LPR = decltype(lpr)::value, RG = 64 / LPR;
        hipLaunchKernelGGL((deepmusic_record_kernel<LPR>), dim3((unsigned)((batch + RG - 1) / RG)), dim3(64), 0, st, table,
                           rows, ids, gen, batch, d, wm, grad_gen, w.rec);
    });
    hipLaunchKernelGGL(deepmusic_loss_kernel, dim3(1), dim3(256), 0, st, w.rec, batch, d, reg, scale, loss_out, w.rinv);
    if (grad_gen) {
        const int64_t quads = batch * (d / 4), blocks = (quads + 255) / 256;
        hipLaunchKernelGGL(deepmusic_gen_add_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st, gen,
                           w.rinv, quads, grad_gen);
    }
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}
