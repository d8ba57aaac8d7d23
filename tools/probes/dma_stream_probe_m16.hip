// The M16 rung of dma_stream_probe.hip: what does the ids side-band DMA of the compacted screen pass cost per tile?
// Stage 1's tile loop (score_topk_dma_kernel<_Float16,128,4,false,true,true>) rebuilt bare: 4 waves x 128 users, 128 AGPRs of B
// fragments, 8 chunks per 32-item tile read by the same eight ds_read_b128 two groups ahead, 64 v_mfma_f32_16x16x32_f16 per tile in
// four groups, two accumulator sets, the maxima in group 0, the barrier and the DMA issue in group 1, the compares in group 2 -- no
// events (the thresholds are never met).  The ids DMA (256 B: one dword per lane) is switched by IDS:
//   0  none                                                               s_waitcnt vmcnt(2) before the barrier
//   1  by every wave in every body (the kernel before round 15)            vmcnt(3)
//   2  every 2nd body by one wave in rotation, strict count               vmcnt(2) everywhere (the issuer waits for ids one tile old)
//   3  every 2nd body by one wave in rotation, counted                    vmcnt(3) in the issuer's next body, vmcnt(2) elsewhere
// Reports the shader clock counter's ticks per tile (over the whole loop, mean of the workgroups) and wall time per launch over
// >= 2 s of back-to-back launches on random operands: dma_stream_probe_m16 [tiles per launch] [seconds per rung].
// hipcc --offload-arch=gfx950 -O3 -mllvm -amdgpu-mfma-vgpr-form -o dma_stream_probe_m16 dma_stream_probe_m16.hip
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <type_traits>
#include <vector>
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float max8(const f32x8& v) {
    float a0, a1, a2, r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(a0) : "v"(v[0]), "v"(v[1]), "v"(v[2]));
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(a1) : "v"(v[3]), "v"(v[4]), "v"(v[5]));
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(a2) : "v"(v[6]), "v"(v[7]), "v"(a0));
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a1), "v"(a2));
    return r;
}

template <int IDS>
__global__ __launch_bounds__(256, 1) void k(const char* __restrict__ tiles, int n_tiles_buf, const int* __restrict__ ids, float* out,
                                           int n_tiles, unsigned long long* clk) {
    constexpr int NCH = 8, NU = 8, TILE_B = NCH * 1024, RING = 4, GR = 2, NG = 4, BG = 1, TG = 2, CPW = 2, BQ = 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    f32x4 b[BQ][NU];
    for (int q = 0; q < BQ; ++q)
        for (int u = 0; u < NU; ++u)
            b[q][u] = *reinterpret_cast<const f32x4*>(tiles + ((size_t)((wave * 31 + q * NU + u) * 64 % 4096) + lane) * 16);
    for (int q = 0; q < BQ; ++q)
        for (int u = 0; u < NU; ++u) asm volatile("" : "+a"(b[q][u]));
    char* ring = smem;
    unsigned* idl = reinterpret_cast<unsigned*>(smem + RING * TILE_B);   // [9][32] ids, as the kernel's
    const char* mine = tiles + (wave * CPW) * 1024 + lane * 16;
    const int tbase = blockIdx.x / 32 * 131;                              // the workgroups of an XCD-sized group walk the same tiles
    auto dma_tile = [&](int j, int slot) __attribute__((always_inline)) {
        const int t = (tbase + j) % n_tiles_buf;
        const char* g = mine + (size_t)t * TILE_B;
        char* l = ring + slot * TILE_B + (wave * CPW) * 1024;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)l, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)l, 16, 1024, 0);
    };
    auto dma_ids = [&](int j) __attribute__((always_inline)) {
        const int t = (tbase + j) % n_tiles_buf;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ids + ((unsigned)t << 5) + lane),
                                         (__attribute__((address_space(3))) void*)(idl + (j & 7) * 32), 4, 0, 0);
    };
    f32x8 acc[2][NU];
    for (int p = 0; p < 2; ++p)
        for (int u = 0; u < NU; ++u)
            for (int r = 0; r < 8; ++r) acc[p][u][r] = 0.0f;
    float thr[NU];
    for (int u = 0; u < NU; ++u) thr[u] = 1e30f;
    f32x4 c[4][GR];
    const uint32_t ring_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)ring + (lane >> 5) * 1024 +
                              ((lane >> 4) & 1) * 512 + (lane & 15) * 16;
    auto rd = [&](f32x4(&dst)[GR], uint32_t addr, auto Gc) __attribute__((always_inline)) {
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst[0]) : "v"(addr), "i"(decltype(Gc)::value * GR * 1024));
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst[1]) : "v"(addr), "i"(decltype(Gc)::value * GR * 1024 + 256));
    };
    auto wt = [&](f32x4(&x)[GR]) __attribute__((always_inline)) { asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(x[0]), "+v"(x[1])); };
    unsigned hits = 0;
    auto body = [&](auto Pc, int j, int s_cur, int s_nxt, int s_fill) __attribute__((always_inline)) {
        constexpr int P = decltype(Pc)::value, Q = 1 - P;
        const uint32_t src = ring_lds + s_cur * TILE_B, srcn = ring_lds + s_nxt * TILE_B;
        const bool my_turn = wave == ((j >> 1) & 3);      // scalar: the ids issuer of this loop trip (IDS 2, 3)
        float m[NU];
        auto group = [&](auto Gc) __attribute__((always_inline)) {
            constexpr int g = decltype(Gc)::value;
            if constexpr (g + 2 < NG) rd(c[(g + 2) & 3], src, std::integral_constant<int, g + 2>{});
            else rd(c[(g + 2) & 3], srcn, std::integral_constant<int, g + 2 - NG>{});
            if constexpr (g == BG) {
                if constexpr (IDS == 1) {
                    asm volatile("s_waitcnt vmcnt(%0)" ::"i"(CPW + 1) : "memory");
                } else if constexpr (IDS == 3 && P == 1) {
                    if (my_turn) asm volatile("s_waitcnt vmcnt(%0)" ::"i"(CPW + 1) : "memory");
                    else asm volatile("s_waitcnt vmcnt(%0)" ::"i"(CPW) : "memory");
                } else {
                    asm volatile("s_waitcnt vmcnt(%0)" ::"i"(CPW) : "memory");
                }
                __builtin_amdgcn_s_barrier();
            }
            __builtin_amdgcn_sched_barrier(0);
            wt(c[g & 3]);
            if constexpr (g == BG) {
                if constexpr (IDS == 1) dma_ids(j + 3);
                if constexpr (IDS >= 2 && P == 0) {
                    if (my_turn) dma_ids(j + 3);
                }
                dma_tile(j + 3, s_fill);
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x004, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);
                }
            }
            if constexpr (g == 0) {
#pragma unroll
                for (int u = 0; u < NU; ++u)
#pragma unroll
                    for (int r = 0; r < 8; ++r) acc[P][u][r] = 0.0f;
            }
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) {
                const f16x8 ca = __builtin_bit_cast(f16x8, c[g & 3][mb]);
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    f32x8& x = acc[P][u];
                    f32x4 t = mb ? f32x4{x[4], x[5], x[6], x[7]} : f32x4{x[0], x[1], x[2], x[3]};
                    t = __builtin_amdgcn_mfma_f32_16x16x32_f16(ca, __builtin_bit_cast(f16x8, b[g][u]), t, 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < 4; ++r) x[4 * mb + r] = t[r];
                }
            }
            if constexpr (g == 0) {
#pragma unroll
                for (int u = 0; u < NU; ++u) m[u] = max8(acc[Q][u]);
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
                }
            }
            unsigned long long hitm = 0ull;
            if constexpr (g == TG) {
#pragma unroll
                for (int u = 0; u < NU; ++u) hitm |= __ballot(m[u] > thr[u]);
#pragma unroll
                for (int q = 0; q < NU; ++q) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x004, 1, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (g == TG) {
                if (hitm != 0ull && j > 0) hits += idl[((j - 1) & 7) * 32 + (lane & 31)];   // never: the event's one LDS read
            }
        };
        [&]<int... Gs>(std::integer_sequence<int, Gs...>) __attribute__((always_inline)) {
            (group(std::integral_constant<int, Gs>{}), ...);
        }(std::make_integer_sequence<int, NG>{});
    };
    if (IDS) {
        dma_ids(0);
        dma_ids(2);
    }
    dma_tile(0, 0); dma_tile(1, 1); dma_tile(2, 2);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    rd(c[0], ring_lds, std::integral_constant<int, 0>{});
    rd(c[1], ring_lds, std::integral_constant<int, 1>{});
    const unsigned long long t0 = __builtin_readcyclecounter();
    int s0 = 0;
    for (int j = 0; j < n_tiles; j += 2) {
        const int s1 = (s0 + 1) & 3, s2 = (s0 + 2) & 3, s3 = (s0 + 3) & 3;
        body(std::integral_constant<int, 0>{}, j, s0, s1, s3);
        body(std::integral_constant<int, 1>{}, j + 1, s1, s2, s0);
        s0 = s2;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(c[0][0]), "+v"(c[0][1]), "+v"(c[1][0]), "+v"(c[1][1]), "+v"(c[2][0]), "+v"(c[2][1]),
                 "+v"(c[3][0]), "+v"(c[3][1]));
    const unsigned long long t1 = __builtin_readcyclecounter();
    float s = (float)hits;
    for (int p = 0; p < 2; ++p)
        for (int u = 0; u < NU; ++u)
            for (int r = 0; r < 8; ++r) s += acc[p][u][r];
    out[blockIdx.x * 256 + threadIdx.x] = s;
    if (threadIdx.x == 0) clk[blockIdx.x] = t1 - t0;
}

constexpr int LDS_BYTES = 4 * 8192 + 9 * 32 * 4;

template <int IDS>
void run(const char* dt, int ntb, const int* ids, float* dout, unsigned long long* dclk, int n_tiles, double seconds, const char* name) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k<IDS>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
    hipLaunchKernelGGL((k<IDS>), dim3(256), dim3(256), LDS_BYTES, 0, dt, ntb, ids, dout, n_tiles, dclk);      // warm-up
    (void)hipDeviceSynchronize();
    int launches = 0;
    double cyc = 0.0;
    const auto w0 = std::chrono::steady_clock::now();
    double wall = 0.0;
    while (wall < seconds) {
        for (int r = 0; r < 8; ++r) hipLaunchKernelGGL((k<IDS>), dim3(256), dim3(256), LDS_BYTES, 0, dt, ntb, ids, dout, n_tiles, dclk);
        (void)hipDeviceSynchronize();
        launches += 8;
        unsigned long long c[256];
        (void)hipMemcpy(c, dclk, sizeof(c), hipMemcpyDeviceToHost);
        double s = 0.0;
        for (int i = 0; i < 256; ++i) s += (double)c[i];
        cyc += s / 256.0;
        wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
    }
    const double ms = wall * 1e3 / launches;
    const double flop = 2.0 * 16 * 16 * 32 * 64.0 * n_tiles * 4 * 256;
    printf("%-62s %8.3f ms per launch (%3d launches)  %.3f of 2.5 PF  %.1f counter ticks per tile  (%s)\n", name, ms, launches,
           flop / ms / 1e9 / 2500, cyc / (launches / 8) / n_tiles, hipGetErrorString(hipGetLastError()));
}

int main(int argc, char** argv) {
    const int n_tiles = argc > 1 ? atoi(argv[1]) : 40000;
    const double seconds = argc > 2 ? atof(argv[2]) : 2.0;
    const int ntb = 65536;                      // 512 MiB of tiles: the stream does not fit any cache
    std::vector<_Float16> h((size_t)4096 * 64 * 8);
    srand(1);
    for (auto& x : h) x = (_Float16)((rand() / (float)RAND_MAX - 0.5f) * 0.2f);
    char* dt;
    int* ids;
    float* dout;
    unsigned long long* dclk;
    (void)hipMalloc(&dt, (size_t)ntb * 8192);
    for (size_t off = 0; off < (size_t)ntb * 8192; off += h.size() * 2) (void)hipMemcpy(dt + off, h.data(), h.size() * 2, hipMemcpyHostToDevice);
    (void)hipMalloc(&ids, (size_t)(ntb + 2) * 32 * 4);
    (void)hipMemset(ids, 0x55, (size_t)(ntb + 2) * 32 * 4);
    (void)hipMalloc(&dout, 256 * 256 * 4);
    (void)hipMalloc(&dclk, 256 * 8);
    for (int rep = 0; rep < 2; ++rep) {
        run<1>(dt, ntb, ids, dout, dclk, n_tiles, seconds, "ids DMA: every wave, every body (before round 15)");
        run<3>(dt, ntb, ids, dout, dclk, n_tiles, seconds, "ids DMA: one wave per 2 bodies, counted vmcnt(3)/(2)");
        run<2>(dt, ntb, ids, dout, dclk, n_tiles, seconds, "ids DMA: one wave per 2 bodies, strict vmcnt(2)");
        run<0>(dt, ntb, ids, dout, dclk, n_tiles, seconds, "ids DMA: none");
    }
    return 0;
}
