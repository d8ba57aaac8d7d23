// The M16 rung of dma_stream_probe.hip: what does the ids side-band DMA of the compacted screen pass cost per tile?
// Stage 1's tile loop (score_topk_dma_kernel<_Float16,128,4,false,true,true>) rebuilt bare: 4 waves x 128 users, 128 AGPRs of B
// fragments, 8 chunks per 32-item tile read by the same eight ds_read_b128 two groups ahead, 64 v_mfma_f32_16x16x32_f16 per tile in
// four groups, two accumulator sets, the maxima in group 0, the barrier and the DMA issue in group 1, the compares in group 2 -- no
// events (the thresholds are never met).  The ids DMA (256 B: one dword per lane) is switched by IDS:
//   0  none                                                               s_waitcnt vmcnt(2) before the barrier
//   1  by every wave in every body (the kernel before round 15)            vmcnt(3)
//   2  every 2nd body by one wave in rotation, strict count               vmcnt(2) everywhere (the issuer waits for ids one tile old)
//   3  every 2nd body by one wave in rotation, counted                    vmcnt(3) in the issuer's next body, vmcnt(2) elsewhere
// Round 16 added two rungs on the IDS = 1 form: the same placement with the tile index clamped as the kernel clamps it (the modulo
// by a run-time divisor is the probe's own cost), and kh, the HOOKED placement of the kernel's body16 (see there).
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

template <int IDS, bool CL = false>
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
        const int t = CL ? (tbase + j < n_tiles_buf ? tbase + j : n_tiles_buf - 1) : (tbase + j) % n_tiles_buf;
        const char* g = mine + (size_t)t * TILE_B;
        char* l = ring + slot * TILE_B + (wave * CPW) * 1024;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)l, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)l, 16, 1024, 0);
    };
    auto dma_ids = [&](int j) __attribute__((always_inline)) {
        const int t = CL ? (tbase + j < n_tiles_buf ? tbase + j : n_tiles_buf - 1) : (tbase + j) % n_tiles_buf;
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

// The HOOKED placement (round 16): the same tile, ring, barrier, DMAs, maxima and compares, the same 64 MFMAs in the same order, but
// every MFMA is followed by one explicit slot, fenced by sched_barrier(0), so that what the source puts into a gap stands there in the
// listing.  Budget per gap: 8 issue cycles beside the MFMA (two 4-cycle vector instructions, or one vector and one or two scalar); a
// ds_read_b128 or a DMA has a gap to itself.
//   group 0   gaps 0..15   two of tile j-1's 32 maxima each
//   group 1   (vmcnt, barrier, lgkmcnt in front)  gap 0 the tile index, 1 ids address, 2 ids DMA, 3 tile address, 4/5 the two pieces,
//             8/9 the fragment reads of group 3
//   group 2   gaps 0..7 one compare and its s_or each, 8/9 the fragment reads of tile j+1's group 0, 10.. the next trip's ring address
//   group 3   gaps 0/1 and 6/7 the fragment reads of tile j+1's groups 1 and 2
// The ring slot is j & 3 (bodies unrolled by two: one scalar offset per trip, +TILE_B by immediate), body 0 is peeled (no j > 0 in
// the tail), the tile index is clamped as in the kernel.  Fragment reads are issued in the order g0 g1 g2 (tile j+1) g3 (tile j), two
// each: the counted waits in front of groups 0..3 are lgkmcnt(4), (2), (2), (2).
__global__ __launch_bounds__(256, 1) void kh(const char* __restrict__ tiles, int n_tiles_buf, const int* __restrict__ ids, float* out,
                                             int n_tiles, unsigned long long* clk) {
    constexpr int NCH = 8, NU = 8, TILE_B = NCH * 1024, RING = 4, NG = 4, BG = 1, TG = 2, CPW = 2, BQ = 4;
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
    unsigned* idl = reinterpret_cast<unsigned*>(smem + RING * TILE_B);
    const unsigned voff = (unsigned)((wave * CPW) * 1024 + lane * 16);   // this lane's 16 bytes of the wave's pieces of a tile
    const int tbase = blockIdx.x / 32 * 131;
    f32x8 acc[2][NU];
    for (int p = 0; p < 2; ++p)
        for (int u = 0; u < NU; ++u)
            for (int r = 0; r < 8; ++r) acc[p][u][r] = 0.0f;
    float thr[NU];
    for (int u = 0; u < NU; ++u) thr[u] = 1e30f;
    f32x4 c[4][2];
    const uint32_t ring_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)ring + (lane >> 5) * 1024 +
                              ((lane >> 4) & 1) * 512 + (lane & 15) * 16;
    auto rd1 = [&](f32x4& dst, uint32_t addr, auto Oc) __attribute__((always_inline)) {
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(decltype(Oc)::value));
    };
    auto wt = [&](f32x4(&x)[2], auto Nc) __attribute__((always_inline)) {
        asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(x[0]), "+v"(x[1]) : "i"(decltype(Nc)::value));
    };
    unsigned hits = 0;
    uint32_t A = ring_lds;       // LDS base of the trip's first tile: ring slot j & 2; moved on in body 1 behind its last use
    // body P of the trip: tile j in slot (j & 2) + P.  FIRST: the peeled body 0 (no tile in front of it to test)
    auto body = [&](auto Pc, auto Fc, int j) __attribute__((always_inline)) {
        constexpr int P = decltype(Pc)::value, Q = 1 - P;
        constexpr bool FIRST = decltype(Fc)::value;
        float m[NU], a0[NU], a1[NU], a2[NU];
        unsigned long long hitm = 0ull;
        int t = 0;
        const int* gi = ids;
        const char* gt = tiles;
        unsigned fill_off = 0;
        auto hook = [&](auto Gc, auto Nc) __attribute__((always_inline)) {
            constexpr int g = decltype(Gc)::value, n = decltype(Nc)::value;
            if constexpr (g == 0 && !FIRST) {
                constexpr int u = n >> 1;
                const f32x8& v = acc[Q][u];
                if constexpr ((n & 1) == 0) {
                    asm volatile("v_max3_f32 %0, %1, %2, %3" : "=v"(a0[u]) : "v"(v[0]), "v"(v[1]), "v"(v[2]));
                    asm volatile("v_max3_f32 %0, %1, %2, %3" : "=v"(a1[u]) : "v"(v[3]), "v"(v[4]), "v"(v[5]));
                } else {
                    asm volatile("v_max3_f32 %0, %1, %2, %3" : "=v"(a2[u]) : "v"(v[6]), "v"(v[7]), "v"(a0[u]));
                    asm volatile("v_max_f32 %0, %1, %2" : "=v"(m[u]) : "v"(a1[u]), "v"(a2[u]));
                }
            }
            if constexpr (g == BG) {
                if constexpr (n == 0) {
                    t = tbase + j + 3;
                    t = t < n_tiles_buf ? t : n_tiles_buf - 1;
                    // body 0 fills the slot of tile j-1 = (j & 2 ^ 2) + 1, body 1 that of tile j-1 = j & 2 (j its own, odd, index)
                    fill_off = (unsigned)(P ? (j & 2) : ((j & 2) ^ 2) + 1) * TILE_B;
                }
                if constexpr (n == 1) gi = ids + ((unsigned)t << 5) + lane;
                if constexpr (n == 2)
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gi,
                                                     (__attribute__((address_space(3))) void*)(idl + ((j + 3) & 7) * 32), 4, 0, 0);
                if constexpr (n == 3) gt = tiles + (size_t)t * TILE_B + voff;
                if constexpr (n == 4)
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gt,
                                                     (__attribute__((address_space(3))) void*)(ring + fill_off + (wave * CPW) * 1024), 16, 0, 0);
                if constexpr (n == 5)
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gt,
                                                     (__attribute__((address_space(3))) void*)(ring + fill_off + (wave * CPW) * 1024), 16, 1024, 0);
                if constexpr (n == 8) rd1(c[3][0], A, std::integral_constant<int, P * TILE_B + 3 * 2048>{});
                if constexpr (n == 9) rd1(c[3][1], A, std::integral_constant<int, P * TILE_B + 3 * 2048 + 256>{});
                // body 1: the trip's base has had its last use; the next trip's tiles (and this body's look-ahead) start at slot (j + 1) & 2
                if constexpr (n == 10 && P == 1) A = ring_lds + (unsigned)((j + 1) & 2) * TILE_B;
            }
            if constexpr (g == TG) {
                if constexpr (n < NU && !FIRST) hitm |= __ballot(m[n] > thr[n]);
                // tile j+1: body 0 -> the same base + TILE_B, body 1 -> the base just moved on
                if constexpr (n == 8) rd1(c[0][0], A, std::integral_constant<int, (P ? 0 : TILE_B)>{});
                if constexpr (n == 9) rd1(c[0][1], A, std::integral_constant<int, (P ? 0 : TILE_B) + 256>{});
            }
            if constexpr (g == 3) {
                if constexpr (n == 0) rd1(c[1][0], A, std::integral_constant<int, (P ? 0 : TILE_B) + 2048>{});
                if constexpr (n == 1) rd1(c[1][1], A, std::integral_constant<int, (P ? 0 : TILE_B) + 2048 + 256>{});
                if constexpr (n == 6) rd1(c[2][0], A, std::integral_constant<int, (P ? 0 : TILE_B) + 2 * 2048>{});
                if constexpr (n == 7) rd1(c[2][1], A, std::integral_constant<int, (P ? 0 : TILE_B) + 2 * 2048 + 256>{});
            }
        };
        auto group = [&](auto Gc) __attribute__((always_inline)) {
            constexpr int g = decltype(Gc)::value;
            if constexpr (g == BG) {
                asm volatile("s_waitcnt vmcnt(%0)" ::"i"(CPW + 1) : "memory");
                __builtin_amdgcn_s_barrier();
            }
            __builtin_amdgcn_sched_barrier(0);
            wt(c[g], std::integral_constant<int, (g == 0 ? 4 : 2)>{});
            __builtin_amdgcn_sched_barrier(0);
            [&]<int... N>(std::integer_sequence<int, N...>) __attribute__((always_inline)) {
                (([&]() __attribute__((always_inline)) {
                     constexpr int mb = N >> 3, u = N & 7;
                     f32x8& x = acc[P][u];
                     f32x4 tt = mb ? f32x4{x[4], x[5], x[6], x[7]} : f32x4{x[0], x[1], x[2], x[3]};
                     if constexpr (g == 0) tt = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                     tt = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, c[g][mb]), __builtin_bit_cast(f16x8, b[g][u]), tt, 0, 0, 0);
#pragma unroll
                     for (int r = 0; r < 4; ++r) x[4 * mb + r] = tt[r];
                     __builtin_amdgcn_sched_barrier(0);
                     hook(Gc, std::integral_constant<int, N>{});
                     __builtin_amdgcn_sched_barrier(0);
                 }()),
                 ...);
            }(std::make_integer_sequence<int, 16>{});
            if constexpr (g == TG && !FIRST) {
                if (hitm != 0ull) hits += idl[((j - 1) & 7) * 32 + (lane & 31)];   // never: the event's one LDS read
            }
        };
        [&]<int... Gs>(std::integer_sequence<int, Gs...>) __attribute__((always_inline)) {
            (group(std::integral_constant<int, Gs>{}), ...);
        }(std::make_integer_sequence<int, NG>{});
    };
    // prologue as the present rung's: ids of tiles 0 .. 3, tiles 0 .. 2
    for (int p = 0; p < 2; ++p)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ids + ((unsigned)(tbase + 2 * p) << 5) + lane),
                                         (__attribute__((address_space(3))) void*)(idl + 2 * p * 32), 4, 0, 0);
    for (int p = 0; p < 3; ++p) {
        const char* g = tiles + (size_t)(tbase + p) * TILE_B + voff;
        char* l = ring + p * TILE_B + (wave * CPW) * 1024;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)l, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)l, 16, 1024, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    rd1(c[0][0], ring_lds, std::integral_constant<int, 0>{});
    rd1(c[0][1], ring_lds, std::integral_constant<int, 256>{});
    rd1(c[1][0], ring_lds, std::integral_constant<int, 2048>{});
    rd1(c[1][1], ring_lds, std::integral_constant<int, 2048 + 256>{});
    rd1(c[2][0], ring_lds, std::integral_constant<int, 2 * 2048>{});
    rd1(c[2][1], ring_lds, std::integral_constant<int, 2 * 2048 + 256>{});
    const unsigned long long t0 = __builtin_readcyclecounter();
    body(std::integral_constant<int, 0>{}, std::true_type{}, 0);
    body(std::integral_constant<int, 1>{}, std::false_type{}, 1);
    for (int j = 2; j < n_tiles; j += 2) {
        body(std::integral_constant<int, 0>{}, std::false_type{}, j);
        body(std::integral_constant<int, 1>{}, std::false_type{}, j + 1);
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

using kern_t = void (*)(const char*, int, const int*, float*, int, unsigned long long*);
void run(kern_t kern, const char* dt, int ntb, const int* ids, float* dout, unsigned long long* dclk, int n_tiles, double seconds, const char* name) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
    hipLaunchKernelGGL(kern, dim3(256), dim3(256), LDS_BYTES, 0, dt, ntb, ids, dout, n_tiles, dclk);      // warm-up
    (void)hipDeviceSynchronize();
    int launches = 0;
    double cyc = 0.0;
    const auto w0 = std::chrono::steady_clock::now();
    double wall = 0.0;
    while (wall < seconds) {
        for (int r = 0; r < 8; ++r) hipLaunchKernelGGL(kern, dim3(256), dim3(256), LDS_BYTES, 0, dt, ntb, ids, dout, n_tiles, dclk);
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
        run(k<1>, dt, ntb, ids, dout, dclk, n_tiles, seconds, "ids DMA: every wave, every body (the kernel's)");
        run(k<3>, dt, ntb, ids, dout, dclk, n_tiles, seconds, "ids DMA: one wave per 2 bodies, counted vmcnt(3)/(2)");
        run(k<2>, dt, ntb, ids, dout, dclk, n_tiles, seconds, "ids DMA: one wave per 2 bodies, strict vmcnt(2)");
        run(k<0>, dt, ntb, ids, dout, dclk, n_tiles, seconds, "ids DMA: none");
        run(k<1, true>, dt, ntb, ids, dout, dclk, n_tiles, seconds, "every wave, every body; tile index clamped, not modulo");
        run(kh, dt, ntb, ids, dout, dclk, n_tiles, seconds, "the same, HOOKED: one slot per MFMA gap (round 16)");
    }
    return 0;
}
