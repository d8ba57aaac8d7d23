// One propagation layer of NGCF (reference model/NGCF.py:94-99), forward and backward, over ALL n_rows rows of the table:
//
//   forward    z = s Wgc^T + bgc + (x (.) s) Wbi^T + bbi,  x_k = leaky_relu(z, 0.01),  acc_out = (acc_in s_in + x_k) s_out
//   backward   dz = g (.) slope(x_k)            (slope = 1 where x_k > 0, else 0.01: the sign of x_k is the sign of z)
//              T = dz Wbi,  ds = dz Wgc + x (.) T,  local = c dOUT + s (.) T
//              dWgc = dz^T s,  dWbi = dz^T (x (.) s),  db = column sums of dz
//
// with s = A x the SpMM's output.  Everything is fp32 on v_mfma_f32_32x32x2_f32 (exact fp32 fma chains), plain launches
// on one stream, no atomics; every sum runs in an order fixed by (n_rows, d): two identical calls give identical bits.
//
// Tiles.  A wave owns 32-row tiles of the table, ngcf_tpw(n_rows) consecutive tiles per wave (so that at most 2048 waves
// exist: the number of weight-gradient partials), four waves per workgroup.  K (= d, or 2 d for the stacked forward
// operand [s | x (.) s]) is padded with zeros up to DP = ceil32(d) in registers: a lane's 16-byte piece of a row is
// either whole or absent, since d % 4 == 0.  x (.) s only ever exists in registers.
//
//   forward    lane (li, h) loads the pieces [8 g + 4 h, +4) of row li of x and s -- the A operand of the MFMA as it
//              stands -- and of row o = 32 q + li of Wgc and Wbi -- the B operand.  The stacked weights lie in LDS,
//              zero-padded, up to DP = 64 (34 KB); wider ones are read through L1 / L2, where they stay since every
//              workgroup reads the same 2 d x d floats.  acc[q][r] = z[n0 + crow(r, h)][32 q + li]: the epilogue's
//              loads and stores are 128 contiguous bytes per row and register.
//   backward   phase W (weight gradients): the K index of the MFMA is the row of the tile, A = dz^T, B = [s | x (.) s],
//              both read as one float per lane from rows 2 st + h; the d x 2 d accumulator stays in registers over all
//              the wave's tiles and is written once, as partial number (wave) of the workspace.  Up to DP = 64 it is 128
//              registers; wider ones are cut into CS column / row slabs of at most 8 accumulator tiles, the slab being
//              blockIdx.x (so that the slabs of one row block run together and share its rows in L2).
//              phase D (ds and the local part): dz's pieces in registers as the A operand, B = one float per lane of
//              Wgc / Wbi rows 8 g + 4 h + j (LDS up to DP = 64), two accumulators (dz Wgc, T) per 32 output columns.
//              Up to DP = 64 one kernel runs phase W and then phase D per tile: every input is read from HBM once.
//              Wider: one launch of phase W over the slabs, then one of phase D.  In both forms a tile's g and s are
//              read for the last time before the tile's local and ds are written, by the wave that owns the tile: local
//              may alias g, ds may alias s.
//   reduce     two small kernels add the partials: chunks of 32 consecutive partials, then the chunk sums, in order.
#include "loss_common.h"

namespace {

constexpr int NGCF_MAX_PARTS = 2048;     // waves of a launch = weight-gradient partials
constexpr int NGCF_CHUNK = 32;           // partials per first-stage sum
constexpr float NGCF_SLOPE = 0.01f;      // F.leaky_relu's default

__host__ __device__ inline int64_t ngcf_tiles(int64_t n_rows) { return (n_rows + 31) / 32; }
// 32-row tiles per wave: a function of n_rows alone
__host__ __device__ inline int ngcf_tpw(int64_t n_rows) {
    const int64_t t = (ngcf_tiles(n_rows) + NGCF_MAX_PARTS - 1) / NGCF_MAX_PARTS;
    return t < 1 ? 1 : (int)t;
}
inline int64_t ngcf_parts(int64_t n_rows) {
    const int tpw = ngcf_tpw(n_rows);
    return (ngcf_tiles(n_rows) + tpw - 1) / tpw;
}
// floats of one partial: [dWgc; dWbi] as (2 DP) x DP, then DP bias sums
inline int64_t ngcf_part_floats(int d) {
    const int64_t dp = ceil32(d);
    return 2 * dp * dp + dp;
}

// how the d x 2 d weight-gradient accumulator is cut for one wave: TB base column tiles (each gives a Wgc and a Wbi
// tile) x OT row tiles per slab, OS row groups, CS slabs in all
template <int DP>
struct NgcfCut {
    static constexpr int NT = DP / 32;
    static constexpr int TB = DP <= 64 ? NT : 1;
    static constexpr int OS = DP <= 128 ? 1 : 2;
    static constexpr int OT = (NT + OS - 1) / OS;
    static constexpr int CS = (NT / TB) * OS;
};

__device__ __forceinline__ float ngcf_dz(float g, float xk) { return xk > 0.f ? g : g * NGCF_SLOPE; }

// ---- forward --------------------------------------------------------------------------------------------------------
template <int DP>
__global__ __launch_bounds__(256) void ngcf_fwd_kernel(const float* x, const float* s, const float* w, const float* b,
                                                       int64_t n_rows, int d, int tpw, float* y, const float* acc_in,
                                                       float s_in, float* acc_out, float s_out) {
    constexpr bool WLDS = DP <= 64;
    constexpr int LDW = DP + 4;                        // LDS row stride (floats): b128 reads spread over the banks
    __shared__ __attribute__((aligned(16))) float wl[WLDS ? 2 * DP * LDW : 4];
    if constexpr (WLDS) {
        for (int e = threadIdx.x * 4; e < 2 * DP * DP; e += 1024) {
            const int row = e / DP, col = e % DP, half = row / DP, o = row % DP;
            *reinterpret_cast<f32x4*>(&wl[row * LDW + col]) =
                lg_load4(w + ((int64_t)half * d + o) * d + col, o < d && col < d);
        }
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, h = lane >> 5, li = lane & 31;
    const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t n_tiles = ngcf_tiles(n_rows);
    int64_t t_end = (gw + 1) * tpw;
    if (t_end > n_tiles) t_end = n_tiles;
    for (int64_t t = gw * tpw; t < t_end; ++t) {
        const int64_t n0 = t * 32, row = n0 + li;
        const bool okr = row < n_rows;
        f32x16 acc[DP / 32];
#pragma unroll
        for (int q = 0; q < DP / 32; ++q) {
            // a zero the compiler cannot see through: with a literal 0 it keeps a second set of accumulators live across
            // the tile loop (twice the AGPRs at DP >= 128, one wave per SIMD less at DP = 32 and 128)
            float zero = 0.f;
            asm volatile("" : "+v"(zero));
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[q][r] = zero;
        }
#pragma unroll 2
        for (int g = 0; g < DP / 8; ++g) {
            const int kc = 8 * g + 4 * h;
            const bool ok = okr && kc < d;
            const f32x4 sv = lg_load4(s + row * d + kc, ok), xv = lg_load4(x + row * d + kc, ok);
            const f32x4 pv = sv * xv;
#pragma unroll
            for (int q = 0; q < DP / 32; ++q) {
                const int o = q * 32 + li;
                f32x4 wg, wb;
                if constexpr (WLDS) {
                    wg = *reinterpret_cast<const f32x4*>(&wl[o * LDW + kc]);
                    wb = *reinterpret_cast<const f32x4*>(&wl[(DP + o) * LDW + kc]);
                } else {
                    const bool okw = o < d && kc < d;
                    wg = lg_load4(w + (int64_t)o * d + kc, okw);
                    wb = lg_load4(w + ((int64_t)d + o) * d + kc, okw);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(sv[j], wg[j], acc[q], 0, 0, 0);
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(pv[j], wb[j], acc[q], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < DP / 32; ++q) {
            const int col = q * 32 + li;
            // the biases are added to the finished sum, not carried through it: where they outweigh the products (small x
            // and s) a chain begun at the bias rounds each of its 2 d steps at the bias's magnitude (9x torch's float32
            // distance at d = 256, x and s of size 0.05)
            const float bias = b && col < d ? b[col] + b[d + col] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t n = n0 + crow(r, h);
                if (n >= n_rows || col >= d) continue;
                const int64_t i = n * d + col;
                const float z = acc[q][r] + bias, v = z > 0.f ? z : z * NGCF_SLOPE;
                if (y) y[i] = v;
                if (acc_out) acc_out[i] = ((acc_in ? acc_in[i] * s_in : 0.f) + v) * s_out;
            }
        }
    }
}

// ---- backward -------------------------------------------------------------------------------------------------------
// MODE 0: phase W then phase D per tile (one slab); 1: phase W only (grid.x = the slabs); 2: phase D only
template <int DP, int MODE>
__global__ __launch_bounds__(256) void ngcf_bwd_kernel(const float* x, const float* s, const float* xk, const float* g,
                                                       const float* dout, float c, const float* w, int64_t n_rows, int d,
                                                       int tpw, float* ds, float* local, float* part, int64_t pe) {
    using Cut = NgcfCut<DP>;
    constexpr bool PW = MODE != 2, PD = MODE != 1;
    constexpr bool WLDS = PD && DP <= 64;
    constexpr int TB = Cut::TB, OT = Cut::OT, OS = Cut::OS, NT = Cut::NT;
    static_assert(MODE != 0 || Cut::CS == 1, "the fused form has one slab");
    __shared__ __attribute__((aligned(16))) float wl[WLDS ? 2 * DP * DP : 4];   // [Wgc; Wbi] zero-padded to (2 DP) x DP
    if constexpr (WLDS) {
        for (int e = threadIdx.x * 4; e < 2 * DP * DP; e += 1024) {
            const int row = e / DP, col = e % DP, half = row / DP, o = row % DP;
            *reinterpret_cast<f32x4*>(&wl[e]) = lg_load4(w + ((int64_t)half * d + o) * d + col, o < d && col < d);
        }
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, h = lane >> 5, li = lane & 31;
    const int64_t gw = (int64_t)blockIdx.y * 4 + (threadIdx.x >> 6);
    const int64_t n_tiles = ngcf_tiles(n_rows);
    int64_t t_end = (gw + 1) * tpw;
    if (t_end > n_tiles) t_end = n_tiles;
    if (gw * tpw >= n_tiles) return;                   // no barrier follows
    const int slab = PW ? (int)blockIdx.x : 0, tbg = slab / OS, oh = slab % OS;

    f32x16 wacc[PW ? OT : 1][PW ? TB : 1][2];
    float dbs[PW ? OT : 1];
    if constexpr (PW) {
#pragma unroll
        for (int ot = 0; ot < OT; ++ot) {
            dbs[ot] = 0.f;
#pragma unroll
            for (int tb = 0; tb < TB; ++tb)
#pragma unroll
                for (int q = 0; q < 2; ++q)
#pragma unroll
                    for (int r = 0; r < 16; ++r) wacc[ot][tb][q][r] = 0.f;
        }
    }

    for (int64_t t = gw * tpw; t < t_end; ++t) {
        const int64_t n0 = t * 32;
        if constexpr (PW) {
#pragma unroll 4
            for (int st = 0; st < 16; ++st) {
                const int64_t n = n0 + 2 * st + h;
                const bool okn = n < n_rows;
                float sv[TB], pv[TB];
#pragma unroll
                for (int tb = 0; tb < TB; ++tb) {
                    const int col = (tbg * TB + tb) * 32 + li;
                    const bool ok = okn && col < d;
                    sv[tb] = ok ? s[n * d + col] : 0.f;
                    pv[tb] = ok ? x[n * d + col] * sv[tb] : 0.f;
                }
#pragma unroll
                for (int ot = 0; ot < OT; ++ot) {
                    const int og = oh * OT + ot;
                    if (og >= NT) continue;            // uniform (the last row group of an odd tile count)
                    const int oc = og * 32 + li;
                    float dz = 0.f;
                    if (okn && oc < d) dz = ngcf_dz(g ? g[n * d + oc] : c * dout[n * d + oc], xk[n * d + oc]);
                    dbs[ot] += dz;
#pragma unroll
                    for (int tb = 0; tb < TB; ++tb) {
                        wacc[ot][tb][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(dz, sv[tb], wacc[ot][tb][0], 0, 0, 0);
                        wacc[ot][tb][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(dz, pv[tb], wacc[ot][tb][1], 0, 0, 0);
                    }
                }
            }
        }
        if constexpr (PD) {
            const int64_t row = n0 + li;
            const bool okr = row < n_rows;
            f32x4 dz[DP / 8];                          // the A operand: row li, columns [8 gi + 4 h, +4)
#pragma unroll
            for (int gi = 0; gi < DP / 8; ++gi) {
                const int kc = 8 * gi + 4 * h;
                const bool ok = okr && kc < d;
                const f32x4 gv = g ? lg_load4(g + row * d + kc, ok) : lg_load4(dout + row * d + kc, ok) * c;
                const f32x4 kv = lg_load4(xk + row * d + kc, ok);
#pragma unroll
                for (int j = 0; j < 4; ++j) dz[gi][j] = ngcf_dz(gv[j], kv[j]);
                if constexpr (DP > 128)                // (bounds the loads in flight: see the weights below)
                    if ((gi & 7) == 7) asm volatile("" ::: "memory");
            }
#pragma unroll 1
            for (int q = 0; q < NT; ++q) {
                const int col = q * 32 + li;
                f32x16 au, at;
#pragma unroll
                for (int r = 0; r < 16; ++r) au[r] = at[r] = 0.f;
                // weights from L2 (DP > 64): the rows of step gi + 1 are loaded before the MFMAs of step gi and no
                // further ahead (the compiler barrier: left alone it hoists every load of the unrolled loop and spills)
                // Addresses: a uniform row pointer (scalar registers) plus one per-lane offset for the whole loop; with a
                // 64-bit address per lane and row the loop-invariant addresses alone would fill the register file.
                float wgn[4], wbn[4];
                const unsigned off0 = (unsigned)(4 * h * d + col);
                auto load_w = [&](int gi) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int ku = 8 * gi + j;     // the lane's row is ku + 4 h
                        const float* rg = w + (int64_t)ku * d;
                        const float* rb = rg + (int64_t)d * d;
                        const bool okw = ku + 4 * h < d && col < d;
                        wgn[j] = okw ? rg[off0] : 0.f;
                        wbn[j] = okw ? rb[off0] : 0.f;
                    }
                };
                if constexpr (!WLDS) load_w(0);
#pragma unroll
                for (int gi = 0; gi < DP / 8; ++gi) {
                    float wg[4], wb[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if constexpr (WLDS) {
                            const int k = 8 * gi + 4 * h + j;
                            wg[j] = wl[k * DP + col];
                            wb[j] = wl[(DP + k) * DP + col];
                        } else {
                            wg[j] = wgn[j];
                            wb[j] = wbn[j];
                        }
                    }
                    if constexpr (!WLDS) {
                        if (gi + 1 < DP / 8) load_w(gi + 1);
                        asm volatile("" ::: "memory");
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        au = __builtin_amdgcn_mfma_f32_32x32x2f32(dz[gi][j], wg[j], au, 0, 0, 0);
                        at = __builtin_amdgcn_mfma_f32_32x32x2f32(dz[gi][j], wb[j], at, 0, 0, 0);
                    }
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t n = n0 + crow(r, h);
                    if (n >= n_rows || col >= d) continue;
                    const int64_t i = n * d + col;
                    const float xv = x[i], sv = s[i], dv = dout[i];
                    ds[i] = au[r] + xv * at[r];
                    local[i] = c * dv + sv * at[r];
                }
            }
        }
    }
    if constexpr (PW) {
        float* p = part + gw * pe;
#pragma unroll
        for (int ot = 0; ot < OT; ++ot) {
            const int og = oh * OT + ot;
            if (og >= NT) continue;
#pragma unroll
            for (int tb = 0; tb < TB; ++tb)
#pragma unroll
                for (int q = 0; q < 2; ++q)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        p[((int64_t)q * DP + og * 32 + crow(r, h)) * DP + (tbg * TB + tb) * 32 + li] = wacc[ot][tb][q][r];
            const float v = dbs[ot] + __shfl_xor(dbs[ot], 32);
            if (tbg == 0 && h == 0) p[(int64_t)2 * DP * DP + og * 32 + li] = v;
        }
    }
}

// out[ch][e] = the sum of in[p][e] over the partials p of chunk ch, in ascending order
__global__ __launch_bounds__(256) void ngcf_chunk_sum_kernel(const float* __restrict__ in, int64_t n_in, int64_t pe,
                                                             float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= pe) return;
    const int64_t lo = (int64_t)blockIdx.y * NGCF_CHUNK;
    int64_t hi = lo + NGCF_CHUNK;
    if (hi > n_in) hi = n_in;
    float a = 0.f;
    for (int64_t p = lo; p < hi; ++p) a += in[p * pe + e];
    out[(int64_t)blockIdx.y * pe + e] = a;
}

// the chunk sums in ascending order -> dw (2 d x d, [dWgc; dWbi]) and db (d)
__global__ __launch_bounds__(256) void ngcf_final_sum_kernel(const float* __restrict__ in, int64_t n_in, int64_t pe, int d,
                                                             int dp, float* __restrict__ dw, float* __restrict__ db) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= pe) return;
    const int64_t mat = (int64_t)2 * dp * dp;
    float* dst;
    if (e < mat) {
        const int64_t row = e / dp, col = e % dp, half = row / dp, o = row % dp;
        if (o >= d || col >= d) return;
        dst = dw + (half * d + o) * d + col;
    } else {
        if (e - mat >= d) return;
        dst = db + (e - mat);
    }
    float a = 0.f;
    for (int64_t p = 0; p < n_in; ++p) a += in[p * pe + e];
    *dst = a;
}

struct NgcfWs {
    float *part, *chunk;
    size_t bytes;
};

NgcfWs ngcf_layout(void* base, int64_t n_rows, int d) {
    const int64_t parts = ngcf_parts(n_rows), pe = ngcf_part_floats(d);
    NgcfWs w;
    WsCarver c(base);
    w.part = c.take(parts * pe);
    w.chunk = c.take((parts + NGCF_CHUNK - 1) / NGCF_CHUNK * pe);
    w.bytes = c.bytes;
    return w;
}

bool ngcf_rows_ok(int64_t n_rows) { return n_rows >= 1 && n_rows <= (1 << 30); }

template <int DP>
void ngcf_launch_fwd(const float* x, const float* s, const float* w, const float* b, int64_t n_rows, int d, float* y,
                     const float* acc_in, float s_in, float* acc_out, float s_out, hipStream_t st) {
    const unsigned wgs = (unsigned)((ngcf_parts(n_rows) + 3) / 4);
    hipLaunchKernelGGL((ngcf_fwd_kernel<DP>), dim3(wgs), dim3(256), 0, st, x, s, w, b, n_rows, d, ngcf_tpw(n_rows), y, acc_in,
                       s_in, acc_out, s_out);
}

template <int DP>
void ngcf_launch_bwd(const float* x, const float* s, const float* xk, const float* g, const float* dout, float c,
                     const float* w, int64_t n_rows, int d, float* ds, float* local, float* part, hipStream_t st) {
    const unsigned wgs = (unsigned)((ngcf_parts(n_rows) + 3) / 4);
    const int tpw = ngcf_tpw(n_rows);
    const int64_t pe = ngcf_part_floats(d);
    if constexpr (NgcfCut<DP>::CS == 1) {
        hipLaunchKernelGGL((ngcf_bwd_kernel<DP, 0>), dim3(1, wgs), dim3(256), 0, st, x, s, xk, g, dout, c, w, n_rows, d, tpw,
                           ds, local, part, pe);
    } else {
        hipLaunchKernelGGL((ngcf_bwd_kernel<DP, 1>), dim3(NgcfCut<DP>::CS, wgs), dim3(256), 0, st, x, s, xk, g, dout, c, w,
                           n_rows, d, tpw, ds, local, part, pe);
        hipLaunchKernelGGL((ngcf_bwd_kernel<DP, 2>), dim3(1, wgs), dim3(256), 0, st, x, s, xk, g, dout, c, w, n_rows, d, tpw,
                           ds, local, part, pe);
    }
}

// f(std::integral_constant<int, DP>) with DP = ceil32(d)
template <class F>
void ngcf_dispatch_dp(int d, F&& f) {
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

extern "C" size_t crh_ngcf_workspace_bytes(int64_t n_rows, int d) {
    if (!ngcf_rows_ok(n_rows) || !lg_width_ok(d)) return 0;
    return ngcf_layout(nullptr, n_rows, d).bytes;
}

extern "C" int crh_ngcf_layer_fwd_f32(const float* x, const float* s, const float* w, const float* b, int64_t n_rows, int d,
                                      float* y, const float* acc_in, float s_in, float* acc_out, float s_out, void* stream) {
    CRH_CHECK_ARG(x && s && w, "crh_ngcf_layer_fwd_f32: NULL x, s or w pointer");
    CRH_CHECK_ARG(y || acc_out, "crh_ngcf_layer_fwd_f32: NULL y and acc_out: nothing to compute");
    LG_CHECK_WIDTH("crh_ngcf_layer_fwd_f32", d);
    CRH_CHECK_ARG(ngcf_rows_ok(n_rows), "crh_ngcf_layer_fwd_f32: n_rows %lld out of [1, 2^30]", (long long)n_rows);
    CRH_CHECK_ARG(lg_aligned16(x, s, w, b, y, acc_in, acc_out), "crh_ngcf_layer_fwd_f32: every pointer must be 16-byte aligned");
    CRH_CHECK_ARG(y != x && y != s && acc_out != x && acc_out != s && (!y || y != acc_out),
                  "crh_ngcf_layer_fwd_f32: an output aliases x or s, or y aliases acc_out");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ngcf_dispatch_dp(d, [&](auto dp) {
        ngcf_launch_fwd<decltype(dp)::value>(x, s, w, b, n_rows, d, y, acc_in, s_in, acc_out, s_out, st);
    });
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

extern "C" int crh_ngcf_layer_bwd_f32(const float* x, const float* s, const float* xk, const float* g, const float* dout,
                                      float c, const float* w, int64_t n_rows, int d, float* ds, float* local, float* dw,
                                      float* db, void* workspace, size_t workspace_bytes, void* stream) {
    CRH_CHECK_ARG(x && s && xk && dout && w, "crh_ngcf_layer_bwd_f32: NULL x, s, xk, dout or w pointer");
    CRH_CHECK_ARG(ds && local && dw && db, "crh_ngcf_layer_bwd_f32: NULL ds, local, dw or db pointer");
    LG_CHECK_WIDTH("crh_ngcf_layer_bwd_f32", d);
    CRH_CHECK_ARG(ngcf_rows_ok(n_rows), "crh_ngcf_layer_bwd_f32: n_rows %lld out of [1, 2^30]", (long long)n_rows);
    CRH_CHECK_ARG(lg_aligned16(x, s, xk, g, dout, w, ds, local, dw, db),
                  "crh_ngcf_layer_bwd_f32: every pointer must be 16-byte aligned");
    CRH_CHECK_ARG(ds != local && ds != x && ds != xk && ds != dout && ds != g && local != x && local != xk && local != s &&
                      local != dout,
                  "crh_ngcf_layer_bwd_f32: ds may alias s only, local may alias g only");
    LG_CHECK_WS("crh_ngcf_layer_bwd_f32", workspace, workspace_bytes, crh_ngcf_workspace_bytes(n_rows, d));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const NgcfWs ws = ngcf_layout(workspace, n_rows, d);
    ngcf_dispatch_dp(d, [&](auto dp) {
        ngcf_launch_bwd<decltype(dp)::value>(x, s, xk, g, dout, c, w, n_rows, d, ds, local, ws.part, st);
    });
    const int64_t parts = ngcf_parts(n_rows), pe = ngcf_part_floats(d), chunks = (parts + NGCF_CHUNK - 1) / NGCF_CHUNK;
    const unsigned eb = (unsigned)((pe + 255) / 256);
    hipLaunchKernelGGL(ngcf_chunk_sum_kernel, dim3(eb, (unsigned)chunks), dim3(256), 0, st, ws.part, parts, pe, ws.chunk);
    hipLaunchKernelGGL(ngcf_final_sum_kernel, dim3(eb), dim3(256), 0, st, ws.chunk, chunks, pe, d, (int)ceil32(d), dw, db);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}
