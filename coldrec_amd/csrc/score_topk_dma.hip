// LDS-DMA form of the fused scoring + top-k workgroup kernel (see the comment on the kernel).  Its own translation unit
// because it is built with -mllvm -amdgpu-mfma-vgpr-form (Makefile): one wave per SIMD owns all 512 registers, the
// accumulators must stay in VGPRs (the threshold test reads them) while the user fragments fill the 256 AGPRs; without
// the flag hipcc puts a one-wave-per-SIMD kernel's accumulators into AGPRs and copies half of the user fragments around.
#include <type_traits>
#include <utility>

#include "score_topk_common.h"

namespace crh_score {
namespace {

constexpr int DMA_NW = 4;           // waves per workgroup (one per SIMD)
constexpr int DMA_UPW = 128;        // users per wave
constexpr int TBITS_B = 2 * 64 * 4; // two blocks of 64 tiles' candidate bits
constexpr int FLAGS_B = 64;         // flag form: ready[<= 8] and done[<= 8] counters of the ring slots
// compacted stream (CM): the ids of a tile's 32 rows ride the DMA stream in the place of the tile bits.  One 256-byte piece per
// body carries the ids of tiles j+3 and j+4 into slots (j+3) & 7 and the one behind it (slot 8 only ever takes that second half).
// When body j issues it every wave has selected tile j-2, and tile j+4 shares a slot with tile j-4: eight slots are enough.
constexpr int IDS_SLOTS = 8;
constexpr int IDS_B = (IDS_SLOTS + 1) * 32 * 4;
// ... and behind the id slots the RATED-TILE flags of this workgroup (ScoreArgs::rated_tiles): two 256-byte pieces of 512 tiles each,
// block ts >> 9 in buffer (ts >> 9) & 1.  Wave 0 fetches block b + 1 from the head of a loop trip once every wave is past the last
// tile of block b - 1 (the trip's own rare path: trip_head), some 448 tiles before the first event that reads it.
constexpr int RT_B = 2 * 256;

// per-wave LDS of the DMA kernel: the lists (scores, ids, fill) and a 192-bit membership filter of each user's rated list.
// The rated-list bounds are read from memory when a candidate's filter says "maybe rated" -- NOT rare where lists are long: an unrated
// candidate hits with probability 1 - e^(-len/192), one in five at the headline's lists.  k = 20: 188 bytes per user,
// 94 KiB per workgroup beside the 64 KiB ring.
constexpr int DMA_FW = 6;           // filter words per user
__host__ __device__ constexpr size_t dma_wave_lds_bytes(int K) {
    return (size_t)DMA_UPW * K * 8 + (size_t)DMA_UPW * 4 + (size_t)DMA_UPW * DMA_FW * 4;
}
__device__ __forceinline__ unsigned rated_hash192(int gi) { return ((((unsigned)gi * 2654435761u) >> 16) * (32u * DMA_FW)) >> 16; }

// The 4 UW MFMAs of one fp32 chunk, as Elem<float>::mma (k pairs in the order x, z, y, w, users interleaved), with
// hook(integral_constant<BASE + i>) run right behind MFMA i: the flag form hangs its few non-MFMA instructions (polls, bumps,
// DMA issue) into single MFMA gaps this way -- an fp32 MFMA runs 64 cycles, a gap hides about a dozen scalar / LDS / VMEM
// instructions, and a block of them in FRONT of a group's MFMAs is paid in full (the first flag form did that: -2 % at
// d=128, -4 % at d=64 on 10 M-item streams against the barrier form).
template <int K>
__device__ __forceinline__ float f4_comp(const f32x4& v) {
    if constexpr (K == 0) return v.x;
    else if constexpr (K == 1) return v.z;
    else if constexpr (K == 2) return v.y;
    else return v.w;
}
template <int UW, int BASE, typename H>
__device__ __forceinline__ void mma_f32_hooked(f32x16 (&acc)[UW], const f32x4& c, const f32x4 (&b)[UW], H&& hook) {
    [&]<int... I>(std::integer_sequence<int, I...>) __attribute__((always_inline)) {
        ((acc[I % UW] = __builtin_amdgcn_mfma_f32_32x32x2f32(f4_comp<I / UW>(c), f4_comp<I / UW>(b[I % UW]), acc[I % UW], 0, 0, 0),
          hook(std::integral_constant<int, BASE + I>{})),
         ...);
    }(std::make_integer_sequence<int, 4 * UW>{});
}

// Slow path of one 32x32 accumulator tile, as tile_slow_path (score_topk_common.h) with every memory round trip of the
// common case removed: the candidate-bitmap bits of the tile come out of LDS (tb: the tile's 32 bits, fetched by DMA with
// the tile stream, see tile_bits_kernel), the membership filter out of LDS too; only a filter hit goes to memory (list
// bounds + search).  While one wave is in here the other three wait at the next barrier, and a memory wait in here would
// also wait for the tile DMAs in flight.
// The insert hands back the user's new threshold out of the registers it holds (+1.0 % against reading it back, same box).
// (Measured and not kept, round 5: one LDS round trip per candidate -- the whole list, its fill and the filter word
// requested together, the insert and the user's new threshold computed from those registers -- ran 2.7 % SLOWER on the
// same box, 0.5316 vs 0.5457 of 2.5 PF: most events end at the "cannot enter" test after three scalar reads.)
// ONE_TRIP (fp32, and the screen's fp16 pass): the candidate's list rides the first batch of LDS reads (fill, list, filter word: one
// wait) and the insert works out of those registers -- at fp32 a candidate above its user's threshold does enter (no rounding ties), so the second round trip
// of the two-step form (fill and list read again by the insert) is paid by nearly every event; on the unseeded public fp16 routes
// most events end at the "cannot enter" test and the lean first batch wins (the round-5 measurement above): the fp16 d=256 kernel
// keeps the two-step form.  (The two-step form at fp32: round 6, profiles/r06_one_trip_event_ab.log.)
// The screen's MARGIN rule (round 19; ScoreArgs::margin).  A user's threshold is the tail of its list; once that tail
// is an item (above CRH_MASKED_SCORE) it is max(tail, L[k-1] - M): k = the call's k (ScoreArgs::screen_k <= K'), M one value per call,
// above twice every user's error bound, so a row below L[k-1] - M has an exact score below the k-th best exact one and need not enter
// any list.  M = +inf switches the rule off: L[k-1] - inf = -inf and the maximum is the tail, the same code.  Every wave holds M in
// one register for the launch (a word of LDS read with each candidate's list was measured: 300 cycles per event, more than the rule
// saved).  The new L[k-1] comes out of the registers the insert already holds, as the new tail does: the list is sorted, so with the
// old entries e1 = L[k-1] <= e2 = L[k-2] it is the MEDIAN of e1, e2 and the candidate wherever the candidate lands (below e1: e1;
// between them: the candidate; above e2: e2) -- two v_readlane, one v_med3_f32, no compare with the insert position.  kc = max(k, 2):
// a call with k = 1 takes its SECOND entry, which is no larger than the first -- a lower threshold, covered by the same proof -- so that
// e2 needs no special case.
// Compiled into the fp16 d=128 kernels only (the screen's launches); every other kernel keeps the tail (MG = false).
// es = the old list (lane l: entry l, every entry below the old fill valid), tail = the new tail, an item's or not.
template <bool MG>
__device__ __forceinline__ float dma_new_tau(float tail, float es, float sc, int kc, float m) {
    float t = tail >= CRH_MASKED_SCORE ? tail : CRH_NEG_INF;      // never above what a masked (-1e9) candidate could beat
    if constexpr (MG) {
        const float e1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, es), kc - 1));
        const float e2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, es), kc - 2));
        const float lk = __builtin_amdgcn_fmed3f(sc, e1, e2);
        // (the maximum as a median with +inf: fmaxf quiets its operands first, one more instruction)
        t = __builtin_amdgcn_fmed3f(t, tail > CRH_MASKED_SCORE ? lk - m : CRH_NEG_INF, __builtin_inff());
    }
    return t;
}

// CRH_SCORE_TIMING (profile build): the memory trips taken inside events -- a hit in the user's filter, then the list bounds and the
// search -- and the cycles spent in them, per wave.  The sums travel down to the candidate as one more argument of the profile build.
#ifdef CRH_PROFILE
struct DmaTripProf { unsigned long long ticks, count; };
#define CRH_TRIP_PARAM , DmaTripProf& tp
#define CRH_TRIP_ARG , tp
#define CRH_TRIP_BEGIN const unsigned long long trip_t0 = a.wave_clock != nullptr ? __builtin_amdgcn_s_memtime() : 0ull
#define CRH_TRIP_END                                                   \
    if (a.wave_clock != nullptr) {                                     \
        tp.ticks += __builtin_amdgcn_s_memtime() - trip_t0;            \
        tp.count += 1;                                                 \
    }
#else
#define CRH_TRIP_PARAM
#define CRH_TRIP_ARG
#define CRH_TRIP_BEGIN
#define CRH_TRIP_END
#endif

// One candidate of an event, shared by the 32x32 and the 16x16 forms of the slow path: the LDS batch read, the "cannot enter"
// test, the rated filter with its bounded search, the insert and the user's new threshold out of registers.  sc / gi = the
// candidate's score and id, bm_masked = its candidate-bitmap bit, ul / slot = its user's column in the wave and slot in the call,
// mine = "this lane holds that user's threshold" (the caller's accumulator layout decides which lanes those are).
// LANE_READ (ONE_TRIP, the 16x16 event): lane l reads entry l whatever K -- lanes >= K read the LDS words behind the user's list (the
// wave's own lists, ids and fills: K + 64 words stay inside them) and nobody uses them; the clamp and the select that blanks the
// lanes >= n cost the event two registers that the 16x16 form does not have.
// MG: the margin rule above (margin = the call's M).
// RT (the compacted stream): rt = "a user of this wave rated a row of the candidate's tile", the wave's bit of the tile's rated-tile flags,
// worked out once per event by the caller.  Clear, the candidate is unrated by construction: no filter word, no search.  Without RT
// the filter is consulted whenever the call has rated lists.
template <bool ONE_TRIP, bool LANE_READ = false, bool MG = false, bool RT = false>
__device__ __forceinline__ void dma_candidate(float sc, int gi, bool bm_masked, int ul, int64_t slot, float* ls, int* li, int* cnt, int K,
                                              const ScoreArgs& a, int lane, const unsigned* rfilter, bool mine, float& tau_reg,
                                              float margin, bool rt CRH_TRIP_PARAM) {
    float* lsu = ls + ul * K;
    int* liu = li + ul * K;
    // one batch of LDS reads: fill, tail entry, filter word
    const unsigned hsh = rated_hash192(gi);
    const int n_raw = cnt[ul];
    const int le = ONE_TRIP ? (LANE_READ ? lane : (lane < K ? lane : K - 1)) : K - 1;   // (ONE_TRIP: lane l reads entry l; the others the tail entry)
    const float ks_raw = lsu[le];
    const int ki_raw = liu[le];
    const unsigned fw_raw = (RT ? rt : a.rated_rowptr != nullptr) ? rfilter[ul * DMA_FW + (hsh >> 5)] : 0u;
    const int n = __builtin_amdgcn_readfirstlane(n_raw);
    if (n >= K) {
        const float ks = ONE_TRIP ? __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ks_raw), K - 1))
                                  : __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, ks_raw)));
        const int ki = ONE_TRIP ? __builtin_amdgcn_readlane(ki_raw, K - 1) : __builtin_amdgcn_readfirstlane(ki_raw);
        if (!crh_better(fmaxf(sc, CRH_MASKED_SCORE), gi, ks, ki)) return;   // cannot enter a full list
    }
    bool masked = bm_masked;
    if (!masked && ((__builtin_amdgcn_readfirstlane(fw_raw) >> (hsh & 31)) & 1u)) {
        CRH_TRIP_BEGIN;
        const int64_t lo = a.rated_rowptr[slot], hi = a.rated_rowptr[slot + 1];
        masked = wave_is_masked_at(gi, lo, hi, a.rated_col, nullptr, lane);
        // every load of the search has landed HERE, inside the branch: left pending on this exit, hipcc guards the
        // join with s_waitcnt vmcnt(0) -- paid by EVERY event, and vmcnt counts the tile DMAs in flight too: the
        // flag form issued them one group (0.8 us) earlier, the barrier form at 256-byte rows in this very group, so an
        // event waited for a DMA round trip (round 6, found in the ISA; tile_slow_path has had the same fix since round 4)
        __builtin_amdgcn_s_waitcnt(0x0f70);
        CRH_TRIP_END
    }
    if (masked) sc = CRH_MASKED_SCORE;
    // wave_list_insert (k <= 64 here) that also hands back the user's NEW threshold out of the registers it already
    // holds -- the k-th entry after the insert is the old (k-1)-th or the candidate -- instead of reading it back
    float es = CRH_NEG_INF;
    int ei = CRH_PAD_IDX;
    if constexpr (ONE_TRIP && LANE_READ) {
        es = ks_raw;       // (lanes >= n hold whatever lies behind the list: every use below is under lane < n, or reads a lane < n)
        ei = ki_raw;
    } else if constexpr (ONE_TRIP) {
        if (lane < n) {
            es = ks_raw;
            ei = ki_raw;
        }
    } else {
        if (lane < n) {
            es = lsu[lane];
            ei = liu[lane];
        }
    }
    const int p = __popcll(__ballot(lane < n && crh_better(es, ei, sc, gi)));
    if (p < K) {
        if (lane >= p && lane < n && lane + 1 < K) {
            lsu[lane + 1] = es;
            liu[lane + 1] = ei;
        }
        const int n2 = n < K ? n + 1 : K;
        if (lane == 0) {
            lsu[p] = sc;
            liu[p] = gi;
            cnt[ul] = n2;
        }
        if (n2 >= K) {
            const float prev = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, es), K >= 2 ? K - 2 : 0));
            const float kth = (p == K - 1) ? sc : prev;
            const float t = dma_new_tau<MG>(kth, es, sc, a.screen_k < 2 ? 2 : a.screen_k, margin);
            if (mine) tau_reg = t;
        }
    }
}

// The event of the 16x16 form (the screen's pass), round 15.  It walks its eight user blocks by the masks the common path has just
// computed (the form that compared every block again: round 15, profiles/r15_event_parts_ab.log, part 2a).
// Its candidate takes the one-trip form of the fp32 kernels: the screen's lists are seeded and the threshold in the register is the
// exact K'-th score, so a candidate above it enters unless it is rated, and the two-step form reads fill and list twice for it
// (the two-step form here: round 15, profiles/r15_event_parts_ab.log, part 2b).
// MFMA shape of the screen's two launches (fp16 d=128; M16 of the kernel): v_mfma_f32_16x16x32_f16, which holds a higher clock on
// this power-limited stream than 32x32x16 at the same cycles per flop.  The approximate scores differ in their last bits (32 products
// per instruction instead of 16); the screen's certificate covers any fp32 accumulation order.  (The 32x32x16 form of these launches:
// round 11, profiles/r11_mfma16_ab.log.)
// The common path of the 16x16 form's tile body is placed by hand (body16 in the kernel): one explicit slot behind each of a tile's 64
// MFMAs.  (The body that left the placement to hipcc's sched_group_barrier pipelines: round 16, profiles/r16_body_ab.log.)
// Round 22 went through the listing of body16's common path; what ships:
//   * the second pair of a block's maxima is one asm statement and the counted fragment waits name no register (the sched_barriers
//     on both sides keep the MFMAs behind them).  As two statements, and with waits that name the fragments they guard, hipcc pads
//     each seam with an s_nop, twelve per tile (that form: round 22, profiles/r22_body_ab.log, step B)
//   * BODY_CARRY: the fetch of tile j + 3 is state carried from tile to tile -- scalar bases plus a 32-bit lane offset, the two LDS
//     slots carried offsets; the DMAs stand in gaps 0 - 2 and the state moves on in the free gaps behind them, at most one vector and
//     two scalar instructions each.  Without it the barrier group works the fetch out from j: clamped tile index, per-lane 64-bit
//     addresses, id slot and ring slot
//   * BODY_STRAIGHT: the event is marked unlikely and the trip's two bounds are worked out (and pinned) in gaps of group 3.  Without it
//     the event is inlined where it is tested and the bounds are tested behind the bodies
// The second and the third are the COMPACTED kernel's alone (BODY_CARRY = BODY_STRAIGHT = CM in the kernel), so both forms of that code
// are live.  In the uncompacted one each of them measured slower than the form before it (a call without a bitmap: +2.2 and +1.9 ms per
// step, profiles/r22_body_ab.log): with its events out of line and four more scalars alive across them hipcc reloads six times as many
// spilled SGPRs inside the loop.
// a test whose branch leaves the common path where `straight` (the kernel's BODY_STRAIGHT) holds
#define CRH_DMA_BODY_RARE(straight, x) ((straight) ? __builtin_expect(!!(x), 0) : (long)!!(x))
// What the 16x16 event executes was shortened once more in round 17; the protocol, the inserts and their order are the same:
//   * the 16x16 kernels are compiled for K' = SCREEN_KP (only the screen launches them; launch_score_dma refuses another k): list
//     addresses, the tail entry's lane and the fill tests are immediates
//   * no per-lane test `slot >= n_users`: a padding column's threshold is +inf from the start and a dead wave's are all +inf (where
//     `tau` is set up in the kernel), and an insert moves its own user's only
//   * the rows left in the selected tile are one scalar per event, not a 64-bit test `item0 + row >= split_end` per candidate
//   * gt_mask8 is one asm statement
// (each of the forms before: round 17, profiles/r17_event_steps_ab.log).
// (Measured and not kept, round 17: the candidate's list reads issued by asm statements at the head of its iteration, in flight under
// the score's select tree, the id and the hash, with one wait in front of the first use.  Nothing at the headline, 202.77 against
// 202.67 ms per step, and +1.4 ms without a bitmap: HISTORY.md, profiles/r17_event_steps_ab.log.)
// Round 18, the FULL-LIST form of the 16x16 event.  While the kernel's prologue copies the seeds, each wave works out one wave-uniform
// flag: every live user slot of the wave holds K' entries.  Lists only grow, so the flag holds for the launch; in the screened route
// it is set by every seeded call (the prefix stage ranks a masked item at -1e9 under its own id, so a seed list is full whenever the
// prefix holds K' rows: its tail may be masked, its threshold -inf).  With the flag set the event takes dma_candidate_full below, and
// a hit block with one hit lane and one row runs its candidate with no loop; with it clear (an unseeded call, a seed list that is
// short all the same) the event of round 17 runs.  (The kernels without the flag, and the full-list form without the straight-line
// dispatch: round 18, profiles/r18_event_steps_ab.log.)
// (Measured and not kept, round 18: the full-list form WITHOUT the tail pre-test -- "cannot enter" read off the placing compare as
// p == K', a second compare only for a masked candidate.  It drops two v_readlane and a scalar crh_better per candidate and ran SLOWER
// on the same box, +0.96 ms per step at the headline on top of the full-list form alone; HISTORY.md,
// profiles/r18_event_steps_ab.log.  Why is not measured.)
// dma_candidate<true, true> for a list that is full (K = the compile-time K'): lane l < K holds entry l, an item; there is no fill to
// read, test or write, and the user's new K-th entry is the old (K-1)-th or the candidate.  The order -- "cannot enter", filter,
// insert -- and what each outcome writes are dma_candidate's with n = K.
template <int K, bool RT>
__device__ __forceinline__ void dma_candidate_full(float sc, int gi, bool bm_masked, int ul, int64_t slot, float* ls, int* li,
                                                   const ScoreArgs& a, int lane, const unsigned* rfilter, bool mine, float& tau_reg,
                                                   float margin, bool rt CRH_TRIP_PARAM) {
    static_assert(K >= 2 && K < 64, "one entry per lane");
    constexpr unsigned long long LIST = (1ull << K) - 1ull;     // lanes >= K read what lies behind the list (LANE_READ of dma_candidate)
    float* lsu = ls + ul * K;
    int* liu = li + ul * K;
    // one batch of LDS reads: entry `lane`, filter word
    const unsigned hsh = rated_hash192(gi);
    const float es = lsu[lane];
    const int ei = liu[lane];
    const unsigned fw_raw = (RT ? rt : a.rated_rowptr != nullptr) ? rfilter[ul * DMA_FW + (hsh >> 5)] : 0u;
    const float ks = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, es), K - 1));
    const int ki = __builtin_amdgcn_readlane(ei, K - 1);
    if (!crh_better(fmaxf(sc, CRH_MASKED_SCORE), gi, ks, ki)) return;   // cannot enter
    bool masked = bm_masked;
    if (!masked && ((__builtin_amdgcn_readfirstlane(fw_raw) >> (hsh & 31)) & 1u)) {
        CRH_TRIP_BEGIN;
        const int64_t lo = a.rated_rowptr[slot], hi = a.rated_rowptr[slot + 1];
        masked = wave_is_masked_at(gi, lo, hi, a.rated_col, nullptr, lane);
        __builtin_amdgcn_s_waitcnt(0x0f70);                     // (the search's loads land inside the branch: see dma_candidate)
        CRH_TRIP_END
    }
    if (masked) sc = CRH_MASKED_SCORE;
    const int p = __popcll(__ballot(crh_better(es, ei, sc, gi)) & LIST);
    if (p < K) {
        if (lane >= p && lane + 1 < K) {
            lsu[lane + 1] = es;
            liu[lane + 1] = ei;
        }
        if (lane == 0) {
            lsu[p] = sc;
            liu[p] = gi;
        }
        const float prev = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, es), K - 2));
        const float kth = (p == K - 1) ? sc : prev;
        const float t = dma_new_tau<true>(kth, es, sc, a.screen_k < 2 ? 2 : a.screen_k, margin);
        if (mine) tau_reg = t;
    }
}

// CM (compacted stream): row q of the stream is the q-th unmasked item; idv = the ids of this tile's rows (lane l: row l & 31),
// read from LDS once per event by the caller.  item0 and split_end stay row numbers; there are no masked rows (tb = 0).
template <bool ONE_TRIP, bool CM, bool MG = false>
__device__ __forceinline__ void tile_slow_path_dma(const f32x16& acc, float& tau_reg, float* ls, int* li, int* cnt, int K,
                                                   int ucol0, int64_t slot0, const ScoreArgs& a, int64_t item0,
                                                   int64_t split_end, int lane, unsigned tb, const unsigned* rfilter, int idv,
                                                   float margin, bool rt CRH_TRIP_PARAM) {
    unsigned cm = gt_mask16(acc, tau_reg);
    // bits of this lane's 16 rows: rows (r&3) + 8*(r>>2) + 4*hh <-> bit r.  Masked rows are packed as zeros: with no negative
    // threshold in the group none of them is a candidate, and the bit shuffling (a dozen VALU instructions) is skipped
    unsigned m16 = 0u;
    if (tb != 0u && __ballot(tau_reg < 0.0f) != 0ull) {          // wave-uniform
        const unsigned x = tb >> (4 * (lane >> 5));
        m16 = (x & 0xFu) | ((x >> 4) & 0xF0u) | ((x >> 8) & 0xF00u) | ((x >> 12) & 0xF000u);
        // a masked candidate scores -1e9: it can only enter a list that is not full (tau = -inf)
        if (tau_reg > CRH_NEG_INF) cm &= ~m16;
    }
    const unsigned bm = cm & m16;
    unsigned long long lanes = __ballot(cm != 0u);
    while (lanes) {
        const int L = __builtin_ctzll(lanes);
        lanes &= lanes - 1;
        unsigned cmL = __builtin_amdgcn_readlane(cm, L);
        const unsigned bmL = __builtin_amdgcn_readlane(bm, L);
        const int jl = L & 31, hh = L >> 5;
        const int64_t slot = slot0 + jl;
        if (slot >= a.n_users) continue;
        const int ul = ucol0 + jl;
        while (cmL) {
            const int r = __builtin_ctz(cmL);
            cmL &= cmL - 1;
            const int64_t il = item0 + (r & 3) + 8 * (r >> 2) + 4 * hh;
            if (il >= split_end) continue;   // clamped duplicate rows of the tail tile
            const float sc = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, pick16u(acc, r)), L));
            int gi;
            if constexpr (CM) gi = __builtin_amdgcn_readlane(idv, (r & 3) + 8 * (r >> 2) + 4 * hh);
            else gi = (int)(a.item_base + il);
            dma_candidate<ONE_TRIP, false, MG, CM>(sc, gi, (bmL >> r) & 1u, ul, slot, ls, li, cnt, K, a, lane, rfilter, (lane & 31) == jl, tau_reg, margin, rt CRH_TRIP_ARG);
        }
    }
    // (no read-back of the thresholds: every insert above updated its user's lanes; padding columns keep their +inf)
}

// The same event for the 16x16x32 form (M16 below): acc = the two 16x16 accumulators of one block of 16 users, element 4 mb + r of
// lane (c = lane & 15, g = lane >> 4) = tile row 16 mb + 4 g + r for user column c; all four g-lanes of a user hold its threshold.
typedef float f32x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ unsigned gt_mask8(const f32x8& v, float t) {   // as gt_mask16
    unsigned m = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    // one statement (round 17): behind each of eight separate ones hipcc puts an s_nop, 24 instructions where these 16 do
#define CRH_GT8(R) "v_cmp_gt_f32 vcc, %" #R ", %9\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc\n\t"
    asm(CRH_GT8(8) CRH_GT8(7) CRH_GT8(6) CRH_GT8(5) CRH_GT8(4) CRH_GT8(3) CRH_GT8(2) "v_cmp_gt_f32 vcc, %1, %9\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc"
        : "+v"(m)
        : "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "v"(v[4]), "v"(v[5]), "v"(v[6]), "v"(v[7]), "v"(t)
        : "vcc");
#undef CRH_GT8
#endif
    return m;
}
// v[r] for a wave-uniform r, as a select tree on scalar conditions: the two halves of an accumulator pair are separate register
// tuples, so there is no register-indexed move to be had as in pick16u.  (NOTE, hipcc 7.2: v[readfirstlane(r)] on this f32x8 was
// compiled to a read of element 0 whatever r -- found in the ISA; every candidate but a tile's first row would have carried a wrong score.)
__device__ __forceinline__ float pick8u(const f32x8& v, int r) {
    const bool b0 = r & 1, b1 = r & 2, b2 = r & 4;
    const float p0 = b0 ? v[1] : v[0], p1 = b0 ? v[3] : v[2], p2 = b0 ? v[5] : v[4], p3 = b0 ? v[7] : v[6];
    const float q0 = b1 ? p1 : p0, q1 = b1 ? p3 : p2;
    return b2 ? q1 : q0;
}
// Compiled for K' = SCREEN_KP.  rows_left = the rows of the selected tile inside the cut, 1 .. 32 (the clamped last tile of a cut holds
// fewer), and gi0 = the id of its row 0 (stream in id order), both worked out once per event by the caller.
// FULL = the wave's lists are all full (round 18): the candidates take dma_candidate_full, and a block with ONE hit lane that holds ONE
// row -- every event of the sparse part of the stream -- runs its candidate straight, with neither loop's header, back edge and zero test.
// No lane is tested for `slot0 + column < n_users`: the thresholds of padding columns and dead waves are +inf (see `tau` in the kernel).
template <bool CM, bool FULL>
__device__ __forceinline__ void tile_slow_path_dma16(const f32x8& acc, float& tau_reg, float* ls, int* li, int* cnt, int ucol0,
                                                     int64_t slot0, const ScoreArgs& a, int rows_left, int gi0, int lane, unsigned tb,
                                                     const unsigned* rfilter, int idv, float margin, bool rt CRH_TRIP_PARAM) {
    constexpr int K = SCREEN_KP;
    unsigned cm = gt_mask8(acc, tau_reg);
    unsigned m8 = 0u;                                             // masked rows of this lane, as in the 32x32 form
    if (tb != 0u && __ballot(tau_reg < 0.0f) != 0ull) {           // wave-uniform
        const int g4 = 4 * (lane >> 4);
        m8 = ((tb >> g4) & 0xFu) | (((tb >> (16 + g4)) & 0xFu) << 4);
        if (tau_reg > CRH_NEG_INF) cm &= ~m8;
    }
    const unsigned bm = cm & m8;
    unsigned long long lanes = __ballot(cm != 0u);
    // row bit r of hit lane L (its row mask cmL's lowest bit, or its only one); bmL = the lane's masked rows
    auto candidate = [&](int L, int r, unsigned bmL) __attribute__((always_inline)) {
        const int jl = L & 15, g = L >> 4;
        const int64_t slot = slot0 + jl;
        const int ul = ucol0 + jl;
        const int row = 16 * (r >> 2) + 4 * g + (r & 3);
        if (row >= rows_left) return;   // clamped duplicate rows of the tail tile
        const float sc = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, pick8u(acc, r)), L));
        int gi;
        if constexpr (CM) gi = __builtin_amdgcn_readlane(idv, row);
        else gi = gi0 + row;
        if constexpr (FULL)
            dma_candidate_full<K, CM>(sc, gi, (bmL >> r) & 1u, ul, slot, ls, li, a, lane, rfilter, (lane & 15) == jl, tau_reg, margin, rt CRH_TRIP_ARG);
        else
            dma_candidate<true, true, true, CM>(sc, gi, (bmL >> r) & 1u, ul, slot, ls, li, cnt, K, a, lane, rfilter, (lane & 15) == jl, tau_reg, margin, rt CRH_TRIP_ARG);
    };
    if constexpr (FULL) {
        // (one s_bcnt1 and a compare.  Not `lanes & (lanes - 1)`: under a bitmap the masked rows may have left no hit lane at all)
        if (__popcll(lanes) == 1) {
            const int L = __builtin_ctzll(lanes);
            const unsigned cmL = __builtin_amdgcn_readlane(cm, L);
            if ((cmL & (cmL - 1)) == 0u) {
                candidate(L, __builtin_ctz(cmL), __builtin_amdgcn_readlane(bm, L));
                return;
            }
        }
    }
    while (lanes) {
        const int L = __builtin_ctzll(lanes);
        lanes &= lanes - 1;
        unsigned cmL = __builtin_amdgcn_readlane(cm, L);
        const unsigned bmL = __builtin_amdgcn_readlane(bm, L);
        while (cmL) {
            const int r = __builtin_ctz(cmL);
            cmL &= cmL - 1;
            candidate(L, r, bmL);
        }
    }
}


// ---------------------------------------------------------------------------------------------------------
// LDS-DMA form of the workgroup kernel for 512-byte rows (fp16 d=256: configs[4]; fp32 d=128: the headline).
// What changes against score_topk_wg_kernel, and why (profiles/r04_z_f16_ceiling.json: two thirds of the matrix
// pipe's cycles were MFMA, the rest ring commits, the per-tile barrier and the threshold test at the end of a tile):
//   * the item stream reaches LDS by DMA (global_load_lds, 16 B per lane, 1 KiB per instruction): no staging
//     registers, no ds_write pass; FOUR ring slots, the fill of a tile is issued two tiles before the barrier that
//     publishes it (one tile of slack measured 7 % slower: the first workgroup of an XCD to ask for a tile waits for the
//     fabric, and the lockstep makes everybody wait with it);
//   * FOUR waves (one per SIMD) of 128 users each instead of eight of 64: an A fragment read from LDS feeds four
//     MFMAs instead of two (half the LDS traffic per flop; the chip is power-limited on fp16 operands).  The B
//     fragments of 128 users are 256 registers: they live in the ACCUMULATOR half of the unified register file
//     (an empty asm with an "a" constraint pins them there; gfx950 MFMAs take A/B operands from AGPRs), the two
//     accumulator SETS, the A fragments and everything else in the 256 VGPRs;
//   * two accumulator sets: the threshold test of tile j-1 (and, rarely, its slow path) is issued between the
//     MFMAs of tile j, so the pipe no longer drains at every tile boundary;
//   * ONE workgroup barrier per tile, in the MIDDLE of the tile's MFMA stream: it publishes tile j+1 (every wave
//     waited for its own DMA pieces first) and frees the slot of tile j-1 for the DMA of tile j+3.  A fragment
//     prefetches run across the tile boundary, so no LDS latency is exposed anywhere in the steady state;
//   * the slow path touches no memory in the common case (tile_slow_path_dma): the tiles' candidate bits ride the DMA
//     stream (64 tiles per 256-byte piece); the rated-list bounds left the LDS and the membership filters shrank to 192
//     bits, which makes room for the fourth ring slot at k <= 20.
// Users, thresholds and lists are per wave exactly as in the other kernels: results are identical.
// The loop runs n_steps + 1 bodies: body j multiplies tile j (the last one a clamped duplicate nobody selects) and
// selects tile j - 1.
//
// FL = the FLAG form (fp32, round 6).  The barrier form above gives the four waves no slack at all: a slow-path event of one
// wave (~0.4 us) is paid by the whole workgroup at the next barrier, and events are what separates the kernel from its bare
// MFMA stream (tools/probes/dma_stream_probe_f32.hip: stream 0.943 / 0.963 of the fp32 peak at d = 64 / 128, kernel 0.884 /
// 0.925; with the barriers ablated the d=64 kernel gets 2.5 of its 3.5 points of event cost back).  Here the ring is
// guarded by two monotonic LDS counters per slot instead:
//   ready[s]  += 1 by every wave when ITS pieces of the tile in slot s have landed (it waits for its own DMA of the body
//                before, a whole tile ago, just before it issues the next one at the head of a body);
//   done[s]   += 1 by every wave when its last fragment read of the tile in slot s has returned.
// A wave reads tile t only once ready = 4 (t / R + 1) and refills the slot of tile t - R only once done = 4 (t / R): all
// dependencies point at earlier tiles, so there is no cycle; the polls are one ds_read_b32 issued a group ahead (it rides
// the counted fragment waits) + v_readfirstlane + a scalar compare, and spin only when a partner really is behind.  With
// R = 4 slots and a prefetch distance of 2 tiles a wave may run (NG - 2) / NG of a tile ahead of the slowest reader and a
// whole tile ahead of the slowest refiller: several events' worth at fp32 tile times (3.4 / 6.8 us).  fp16 tiles last
// 0.85 us -- less than a DMA round trip -- so the fp16 kernel keeps the barrier form.
//
// CM = the COMPACTED stream (fp16 d=128: the screened route's pass under a candidate bitmap).  The packed copy holds the unmasked
// rows only, in the map's order (ScoreArgs::idmap, n_live).  The tile count, the cuts' bounds and the DMA clamp come from *n_live; the host sized the
// grid, the cuts and the lockstep windows by its upper bound n_items, and every workgroup of a cut walks the same tiles.  A
// candidate's id comes out of the id slots in LDS (IDS_B, in the place of the tile bits: there is no masked row to tell apart);
// lists, filters, seeds and the cuts' merge stay in id space.
//
// M16 = the 16x16x32 MFMA form (fp16 d=128: both launches of the screened route's pass, round 11).  The same tile, the same ring, barrier,
// DMA placement and two accumulator sets; what changes is the register layout.  The chip is power-limited on this stream, and it
// holds a higher clock on v_mfma_f32_16x16x32_f16 than on 32x32x16 at the same matrix-pipe cycles per flop
// (tools/probes/mfma_energy_probe.hip shape, profiles/r11_mfma_shape_probe.log: 1.97 against 1.63 GHz in the bare loop).
//   * users in 8 blocks of 16 columns: lane (c = lane & 15, g = lane >> 4) holds, for block nb and k-step ks, the 16 bytes at offset
//     64 ks + 16 g of the row of user 16 nb + c -- 32 fragments, 128 AGPRs as before; tau[8], the same value in all four g-lanes;
//   * the packed tile is unchanged (chunk q, 16-byte slot 32 h + i = row i, halfs 16 q + 8 h .. + 7); the A fragment of item half
//     mb and k-step ks is row 16 mb + c, halfs 32 ks + 8 g .. + 7 = byte ks 2048 + (g >> 1) 1024 + (g & 1) 512 + mb 256 + c 16: one
//     per-lane base, immediate offsets, one ds_read_b128 per fragment and eight per tile as before, conflict-free;
//   * a group is k-step ks: its two fragments (mb = 0, 1) each feed the 8 independent MFMAs over nb -- 16 MFMAs of 16 cycles;
//   * accumulators acc[set][nb] as f32x8: element 4 mb + r of lane (c, g) = tile row 16 mb + 4 g + r for user 16 nb + c;
//   * a 16-cycle MFMA hides two other instructions, a 32-cycle one six, so the threshold test is spread: the maxima in group 0,
//     the barrier and the DMA issue in group 1, the compares and the events behind group 2.  (An event reads registers, the id
//     slots and the tile bits of tile j-1, all of which outlive body j: its place inside the body is free.)
//   * since round 16 the common path of this form is `body16` below, placed by hand: one explicit slot behind each MFMA, body 0
//     peeled out of the loop, `live` folded into the thresholds, the ring slot taken from the tile counter.  `body` is the 32x32
//     forms' alone.  (Until round 16 it built this form too and asked hipcc for the same spread by sched_group_barrier pipelines,
//     which do not count the inline-asm maxima as VALU: four maxima stood in front of group 0's first MFMA, the second half of group 2
//     and all of group 3 were bare, and about 25 instructions per tile stood between the groups, hidden by no MFMA.  That body is in
//     history at round 16, profiles/r16_body_ab.log.)
// The approximate scores differ from the 32x32 form's in their last bits (another accumulation order); the screen's results do not
// (stage 2 rescores, and its bound covers any fp32 accumulation order).  The public fp16 routes never run this kernel at d=128.
template <typename T, int D, int R, bool FL, bool CM = false, bool M16 = false>
__global__ __launch_bounds__(256, 1) void score_topk_dma_kernel(ScoreArgs a) {
    constexpr int NW = DMA_NW, UW = 4, UPW = DMA_UPW;
    static_assert(!M16 || (std::is_same<T, _Float16>::value && D == 128 && !FL), "the 16x16x32 form is the fp16 d=128 screen's");
    // register shapes of the two MFMA forms: user blocks of UB columns, NU of them per wave; b[BQ][NU] user fragments (BQ 32-byte
    // chunks, or M16: 64-byte k-steps); accumulators of NR registers per user block (M16: both 16-row halves of the tile in one f32x8)
    constexpr int UB = M16 ? 16 : 32, NU = UPW / UB, NR = M16 ? 8 : 16;
    using AccT = std::conditional_t<M16, f32x8, f32x16>;
    // body j issues the DMA of tile j + PF; in the flag form it publishes its pieces of tile j + PF - 1 (issued one body ago) first:
    // a wave may lead the slowest reader by (NG - 2) / NG of a tile and the slowest refiller by one tile
    constexpr int PF = FL ? 2 : 3;
    static_assert(R == 4 && (!FL || sizeof(T) == 4) && !(CM && FL), "ring shape");
    constexpr int SIDE_B = CM ? IDS_B + RT_B : TBITS_B; // the tile bits' area behind the ring, or the ids' and the rated-tile flags'
    constexpr int ROWB = D * (int)sizeof(T);
    constexpr int NCH = ROWB / 32;
    constexpr int TILE_B = NCH * 1024;
    constexpr int CPW = NCH / NW;                      // 1 KiB DMA pieces of a tile each wave issues
    constexpr int GR = 2, NG = NCH / GR;               // A fragments are read in groups of GR chunks, one group ahead
    constexpr int BG = NG / 2 - 1;                     // the group in front of which the ring barrier sits
    constexpr int TG = M16 ? 2 : 1;                    // the group behind which tile j-1's threshold test (and its events) sits
    constexpr bool BODY_CARRY = CM, BODY_STRAIGHT = CM;   // round 22: both steps measured slower in the uncompacted kernel (see above)
    static_assert(NCH % NW == 0 && NG % 4 == 0 && BG + 2 < NG, "row width not supported by the DMA kernel");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int S = a.n_splits;
    const int split = (int)(blockIdx.x % S);
    const int64_t ug_raw = (int64_t)(blockIdx.x / S) * NW + wave;
    const bool live = ug_raw < a.n_ugroups;            // a dead wave still fetches and synchronises
    const int64_t ug = live ? ug_raw : a.n_ugroups - 1;
    const int K = M16 ? SCREEN_KP : a.k;                // the 16x16 form is compiled for the screen's K' (launch_score_dma checks a.k)
    const int i = lane & (M16 ? 15 : 31), h = lane >> (M16 ? 4 : 5);   // user column in its block, k-group (M16: c and g of the 16x16x32 layout)
    // the screen's launches (fp16 d=128, both MFMA shapes; the public fp16 d=128 calls take another kernel): the margin rule of
    // dma_new_tau
    constexpr bool MG = std::is_same<T, _Float16>::value && D == 128;

    char* ring = smem;                                  // [R][TILE_B]
    unsigned* tbits = reinterpret_cast<unsigned*>(smem + R * TILE_B);   // [2][64]; CM: [IDS_SLOTS + 1][32] ids
    [[maybe_unused]] unsigned* rtiles = tbits + IDS_B / 4;              // CM: [2][64] rated-tile flags of this workgroup
    unsigned* flags = tbits + SIDE_B / 4;             // FL: ready[R] at 0, done[R] at 8; slots of the prologue's tiles start ready
    if constexpr (FL) {
        // (published by the prologue's barrier.  Tiles 0 .. PF-2 of the prologue start complete; tile PF-1 is bumped by body 0 like
        // every tile after it: the prologue waited for all of them)
        if (threadIdx.x < 16) flags[threadIdx.x] = threadIdx.x < PF - 1 ? (unsigned)NW : 0u;
    }
    int64_t n_rows = a.n_items;                          // rows of the stream
    if constexpr (CM) n_rows = (int64_t)__builtin_amdgcn_readfirstlane((int)*a.n_live);
    const int64_t NT = (n_rows + 31) >> 5;
    const int64_t t0 = NT * split / S, t1 = NT * (split + 1) / S;
    const int64_t split_end = (t1 << 5) < n_rows ? (t1 << 5) : n_rows;
    const int64_t slot0w = ug * UPW;
    // ids [lo, hi) of this cut's rows, worked out where they are used (CM: with cuts out of the map, which ascends then, and an
    // empty cut gets an empty range; one cut holds the whole range, in whatever order the map streams it)
    auto cut_ids = [&](int& lo, int& hi) __attribute__((always_inline)) {
        if constexpr (CM) {
            const int id_end = (int)(a.item_base + a.n_items);
            if (S == 1) {
                lo = (int)a.item_base;
                hi = id_end;
            } else {
                lo = (t0 << 5) < n_rows ? a.idmap[t0 << 5] : id_end;
                hi = (t1 << 5) < n_rows ? a.idmap[t1 << 5] : id_end;
            }
        } else {
            lo = (int)(a.item_base + (t0 << 5));
            hi = (int)(a.item_base + split_end);
        }
    };

    // ---- this wave's lists
    char* wl = smem + R * TILE_B + SIDE_B + (FL ? FLAGS_B : 0) + (size_t)wave * dma_wave_lds_bytes(K);
    float* ls = reinterpret_cast<float*>(wl);           // [UPW][K]
    int* li = reinterpret_cast<int*>(ls + UPW * K);      // [UPW][K]
    int* cnt = li + UPW * K;                            // [UPW]
    for (int j = lane; j < UPW; j += 64) cnt[j] = 0;
    [[maybe_unused]] float margin = __builtin_inff();   // MG: the call's M, in one register for the launch
    if constexpr (MG) {
        if (a.margin != nullptr) margin = *a.margin;
    }
    // M16, round 18: every live slot of this wave holds K entries (wave-uniform; lists only grow, so it holds for the launch).  The loop
    // below ends at the first padding slot: padding slots stay empty and do not count -- their thresholds are +inf, no candidate is
    // ever theirs.  (A dead wave copies the lists of the call's last group and takes no event at all.)
    [[maybe_unused]] int lists_full = M16 && a.seed_score != nullptr ? 1 : 0;
    if (a.seed_score) {
        // seeded lists: copy each slot's prefix top-k into LDS; its fill = the entries before the padding
        for (int j = 0; j < UPW; ++j) {
            const int64_t slot = slot0w + j;
            if (slot >= a.n_users) break;                         // wave-uniform
            int n = 0;
            for (int e0 = 0; e0 < K; e0 += 64) {
                const int e = e0 + lane;
                int gi = CRH_PAD_IDX;
                if (e < K) {
                    gi = a.seed_idx[slot * K + e];
                    ls[j * K + e] = a.seed_score[slot * K + e];
                    li[j * K + e] = gi;
                }
                n += __popcll(__ballot(gi != CRH_PAD_IDX));
            }
            if (lane == 0) cnt[j] = n;
            if constexpr (M16) lists_full &= n == K ? 1 : 0;
        }
    }
    // ---- membership filters of the rated lists (192 bits per user, ids of this split's range only)
    unsigned* rfilter = reinterpret_cast<unsigned*>(cnt + UPW);      // [UPW][DMA_FW]
    for (int j = lane; j < UPW * DMA_FW; j += 64) rfilter[j] = 0u;
    if (live && a.rated_rowptr) {
        int id0, id1;
        cut_ids(id0, id1);
        const int64_t s1 = slot0w + UPW < a.n_users ? slot0w + UPW : a.n_users;
        const int64_t e0 = a.rated_rowptr[slot0w], e1 = a.rated_rowptr[s1];
        int64_t nxt = a.rated_rowptr[slot0w + 1];   // end of the list of this lane's current user
        int u = 0;
        for (int64_t base = e0; base < e1; base += 64) {
            const int64_t e = base + lane;
            if (e < e1) {
                const int v = a.rated_col[e];
                while (e >= nxt) { ++u; nxt = a.rated_rowptr[slot0w + u + 1]; }      // entries ascend: terminates at e1
                if (v >= id0 && v < id1) {
                    const unsigned hsh = rated_hash192(v);
                    atomicOr(&rfilter[u * DMA_FW + (hsh >> 5)], 1u << (hsh & 31));
                }
            }
        }
    }

    constexpr int BQ = M16 ? ROWB / 64 : NCH;
    f32x4 b[BQ][NU];
    float tau[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        int64_t slot = slot0w + UB * u + i;
        // padding columns never take a candidate.  The 16x16 event RELIES on this +inf (and on the dead wave's below): it no longer tests
        // `slot < n_users` per hit lane, so nothing but these thresholds keeps a padding column out of a hit mask
        tau[u] = slot < a.n_users ? CRH_NEG_INF : __builtin_inff();
        if (a.seed_score && slot < a.n_users) {
            tau[u] = wave_list_tau(ls + (UB * u + i) * K, cnt[UB * u + i], K);
            if constexpr (MG) {       // a full seed list whose tail is an item: the rule holds from the first tile
                if (cnt[UB * u + i] >= K && ls[(UB * u + i) * K + K - 1] > CRH_MASKED_SCORE)
                    tau[u] = fmaxf(tau[u], ls[(UB * u + i) * K + (a.screen_k < 2 ? 2 : a.screen_k) - 1] - margin);
            }
        }
        if (slot >= a.n_users) slot = a.n_users - 1;
        const int64_t row = a.users ? (int64_t)a.users[slot] : a.user_base + slot;
        const char* up = reinterpret_cast<const char*>(a.user_emb) + row * ROWB + 16 * h;
#pragma unroll
        for (int q = 0; q < BQ; ++q) {
            b[q][u] = load16(up + (M16 ? 64 : 32) * q);      // M16: lane (c, g) holds halfs 32 q + 8 g .. + 7 of user 16 u + c
            if constexpr (Elem<T>::kSwap) chunk_swap(b[q][u]);
        }
    }
    // the 16x16 body tests no `live` per tile: a dead wave walks, synchronises and fetches like any other, and with +inf for
    // every threshold none of its maxima is a hit (it has no list to insert into and stores nothing).  The event relies on it as well:
    // it has no test of its own that would keep a dead wave's lanes out
    if constexpr (M16) {
        if (!live) {
#pragma unroll
            for (int u = 0; u < NU; ++u) tau[u] = __builtin_inff();
        }
    }
    // the user fragments live in AGPRs from here on (and have landed: nothing of theirs is left on the VM counter)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int q = 0; q < BQ; ++q)
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            if constexpr (sizeof(T) == 4) {     // fp32 MFMAs take ONE dword per operand: pinned as a 4-vector hipcc copies every
                asm volatile("" : "+a"(b[q][u].x));   // component to a VGPR first (v_accvgpr_read per MFMA, 23 spills); as four
                asm volatile("" : "+a"(b[q][u].y));   // scalars the MFMA reads a[N] directly
                asm volatile("" : "+a"(b[q][u].z));
                asm volatile("" : "+a"(b[q][u].w));
            } else {
                asm volatile("" : "+a"(b[q][u]));
            }
        }
#endif

    const char* packed = reinterpret_cast<const char*>(a.packed);
    const int n_steps = (int)(t1 - t0);                 // tiles of this split (32-bit loop arithmetic: scalar compares, no VALU)
    // this wave's pieces of step j -> ring slot.  Steps past the split (the extra body, the prefetch distance) read clamped
    // tiles: valid addresses, data nobody selects.
    // One global pointer per lane and ONE LDS base per slot serve the wave's CPW pieces: the instruction's immediate offset
    // moves both addresses (LDS address = M0 + offset + 16 * lane).
    const char* my_pieces = packed + (wave * CPW) * 1024 + lane * 16;
    const int n_tiles32 = (int)NT;                     // item ids are int32, so tiles fit easily
    auto dma_tile = [&](int j, int slot) __attribute__((always_inline)) {
        int t = (int)t0 + j;
        t = t < n_tiles32 ? t : n_tiles32 - 1;
        if (CRH_ABLATE(a.ablate) & 2) t = 0;   // measurement only: every fetch hits the same (cached) tile
        const char* g = my_pieces + (int64_t)t * TILE_B;
        char* l = ring + slot * TILE_B + (wave * CPW) * 1024;
#define CRH_DMA_PIECE(CQ)                                                                                              \
    if constexpr (CQ < CPW)                                                                                            \
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,                             \
                                         (__attribute__((address_space(3))) void*)l, 16, (CQ) * 1024, 0)
        CRH_DMA_PIECE(0); CRH_DMA_PIECE(1); CRH_DMA_PIECE(2); CRH_DMA_PIECE(3);
#undef CRH_DMA_PIECE
        static_assert(CPW <= 4, "pieces beyond the immediate offset range");
    };
    // candidate bits of the 64 tiles of block blk (tile >> 6) -> tbits[blk & 1].  Issued by EVERY wave with EVERY tile (a
    // 256-byte piece; the waves write identical bytes): no branch inside the MFMA stream, one more DMA on everybody's counter.
    // (Round 15 measured the thinned form -- one wave, only where a new piece is due: the stream with no such DMA at all is 1.0 %
    // shorter in cycles per tile, and the scalar branches that thinning needs cost more than that; the headline ran 9 ms slower.
    // DESIGN 4.1.5, profiles/r15_ids_dma_probe.log)
    auto dma_tbits = [&](int64_t blk) __attribute__((always_inline)) {
        int t = ((int)blk << 6) + lane;
        t = t < n_tiles32 ? t : n_tiles32 - 1;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.tile_bits + (unsigned)t),
                                         (__attribute__((address_space(3))) void*)(tbits + (blk & 1) * 64), 4, 0, 0);
    };
    // CM: the ids of tiles t0 + j and t0 + j + 1 -> slots j & 7 and the next one, one id per lane (clamped like the tiles: valid
    // addresses, ids nobody reads).  Issued by every wave with every tile, as the tile bits are
    auto dma_ids = [&](int j) __attribute__((always_inline)) {
        int t = (int)t0 + j;
        t = t < n_tiles32 ? t : n_tiles32 - 1;
        unsigned e = ((unsigned)t << 5) + (unsigned)lane;
        const unsigned e_max = ((unsigned)n_tiles32 << 5) - 1u;
        e = e < e_max ? e : e_max;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.idmap + e),
                                         (__attribute__((address_space(3))) void*)(tbits + (j & (IDS_SLOTS - 1)) * 32), 4, 0, 0);
    };
    // CM: block blk of this workgroup's rated-tile flags -> rtiles[blk & 1], one word per lane (a block past the stream's last one is
    // clamped: valid addresses, flags nobody reads).  Without the flags (or without rated lists) the two buffers are filled once, with
    // ones (every tile takes the filter, as before) or zeros (no lists), and no fetch is ever issued.
    [[maybe_unused]] const bool rt_fetch = CM && a.rated_tiles != nullptr && a.rated_rowptr != nullptr;
    [[maybe_unused]] auto dma_rtiles = [&](int64_t blk) __attribute__((always_inline)) {
        const int64_t nb = screen_rated_blocks(a.n_items);
        const int64_t bc = blk < nb ? blk : nb - 1;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.rated_tiles + (((int64_t)(blockIdx.x / S) * nb + bc) << 6) + lane),
                                         (__attribute__((address_space(3))) void*)(rtiles + (blk & 1) * 64), 4, 0, 0);
    };
    const bool has_bits = !CM && a.bitmap != nullptr;   // without a candidate bitmap tile_bits points at readable filler
    auto dma_wait_all = [&]() __attribute__((always_inline)) {
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    };
    auto dma_wait_but_newest_tile = [&]() __attribute__((always_inline)) {   // everything but the CPW + 1 pieces issued last
#if defined(__HIP_DEVICE_COMPILE__)
        if (CRH_ABLATE(a.ablate) & 16) return;   // measurement only: what the DMA wait costs (results invalid)
        asm volatile("s_waitcnt vmcnt(%0)" ::"i"(CPW + 1) : "memory");
#endif
    };

    AccT acc[2][NU];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
            for (int r = 0; r < NR; ++r) acc[p][u][r] = 0.0f;
    // A fragments: LDS -> registers by inline asm with COUNTED waits.  Left to hipcc the loop gets "s_waitcnt lgkmcnt(0)" right
    // behind the reads of the NEXT group (seen in the ISA: every second group stalls for a full LDS round trip).  The asm reads
    // are invisible to the compiler's counter bookkeeping; lds_wait names the registers it guards, so no MFMA that consumes
    // them can be scheduled above it (cdna_hip_programming.md 5.7: form (ii)).  LDS operations complete in order, so
    // lgkmcnt(2 GR) = "everything but the 2 GR reads issued last has landed" also covers any list access of the slow path.
    f32x4 c[4][GR];
    // M16: the fragment of item half mb and k-step ks wants row 16 mb + c, halfs 32 ks + 8 g .. + 7 in lane (c, g) -- chunk
    // 2 ks + (g >> 1), slot 32 (g & 1) + 16 mb + c of the packed tile: one per-lane base and the immediate offsets ks * 2048 + mb * 256.
    // A group is one k-step, its two fragments the two halves.  (Lanes 0 - 15 of a read are 16 consecutive slots: no bank conflict.)
    const uint32_t ring_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)ring +
                              (M16 ? (lane >> 5) * 1024 + ((lane >> 4) & 1) * 512 + (lane & 15) * 16 : lane * 16);
    auto lds_group = [&](f32x4(&dst)[GR], uint32_t addr, auto Gc) __attribute__((always_inline)) {
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst[0]) : "v"(addr), "i"((decltype(Gc)::value * GR + 0) * 1024));
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst[1]) : "v"(addr), "i"(M16 ? decltype(Gc)::value * GR * 1024 + 256 : (decltype(Gc)::value * GR + 1) * 1024));
#endif
    };
    auto lds_wait = [&](f32x4(&x)[GR], auto Nc) __attribute__((always_inline)) {
#if defined(__HIP_DEVICE_COMPILE__)
        if (CRH_ABLATE(a.ablate) & 8) {          // measurement only: what the fragment waits cost (results invalid)
            asm volatile("" : "+v"(x[0]), "+v"(x[1]));
            return;
        }
        asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(x[0]), "+v"(x[1]) : "i"(decltype(Nc)::value));
#endif
    };
    static_assert(GR == 2, "lds_group / lds_wait are written for two chunks per group");
    // ---- flag form: counters, polls (see the kernel's comment)
    const uint32_t flags_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned*)flags;
    unsigned rflag = 0, dflag = 0;                       // poll results in flight (landed at the next counted fragment wait)
    auto flag_read = [&](unsigned& dst, int word) __attribute__((always_inline)) {
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("ds_read_b32 %0, %1" : "=v"(dst) : "v"(flags_lds + 4u * (unsigned)word));
#endif
    };
    // (all 64 lanes add to the one counter -- lane 0 a one, the others zeros: one instruction and no exec-mask detour; the
    // compiler's form of `if (lane == 0) atomicAdd` is a dozen instructions with two branches)
    const unsigned bump_val = lane == 0 ? 1u : 0u;
    auto flag_bump = [&](int word) __attribute__((always_inline)) {
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("ds_add_u32 %0, %1" ::"v"(flags_lds + 4u * (unsigned)word), "v"(bump_val) : "memory");
#endif
    };
    auto flag_land = [&](unsigned& f) __attribute__((always_inline)) {     // everything LDS issued so far has landed (it was long ago)
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f));
#endif
    };
    // the counted wait of a group in the flag form: everything but the GR fragment reads issued last has landed -- the
    // fragments of this group AND of the next one (a group is 2048 cycles of MFMAs: they landed long ago), the polls, the bumps
    auto lds_wait_fl = [&](f32x4(&x)[GR], unsigned& f0, unsigned& f1) __attribute__((always_inline)) {
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(x[0]), "+v"(x[1]), "+v"(f0), "+v"(f1) : "i"(GR));
#endif
    };
    // spin until counter `word` reaches `want` (rare: a partner wave is behind -- in a slow-path event, or waiting for its XCD)
    auto flag_spin = [&](unsigned have, int word, unsigned want) __attribute__((always_inline)) {
        unsigned v = __builtin_amdgcn_readfirstlane(have);
        if (__builtin_expect(v >= want, 1) || (CRH_ABLATE(a.ablate) & 4)) return;
        unsigned spins = 0;
        do {
            __builtin_amdgcn_s_sleep(1);
            unsigned t;
#if defined(__HIP_DEVICE_COMPILE__)
            asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(t) : "v"(flags_lds + 4u * (unsigned)word) : "memory");
#endif
            v = __builtin_amdgcn_readfirstlane(t);
            if (++spins > (1u << 24)) __builtin_trap();      // seconds: a protocol bug must not hang the GPU (nor pass silently)
        } while (v < want);
    };

#ifdef CRH_PROFILE
    unsigned long long ev_ticks = 0, ev_count = 0;       // CRH_SCORE_TIMING
    DmaTripProf tp = {0ull, 0ull};                       // ... and the memory trips inside the events
    // ... and (round 22, the hooked 16x16 body) the segments of a pair of tiles: a stamp in front of each group and on both sides of
    // the barrier, ten a pair.  Segment 5 b + s of body b (0 the even tile, 1 the odd one): s = 0 group 0, 1 the DMA wait and the
    // barrier, 2 group 1, 3 group 2 with the event's test, 4 group 3 up to the next body's group 0 (the odd body's: with the trip head).
    // A pair's ten are kept apart and added to the wave's sums at the trip head unless an event fell into the pair.  Each stamp is an
    // s_memtime and waits for it with everything LDS in flight, which more than doubles a pair: the stamps are asked for on their own
    // (CRH_SCORE_TIMING=2, the screen's stage 1) and show where the time is; the histogram of a run without them says how much there is.
    unsigned seg_tmp[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, seg_sum[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, seg_pairs = 0;
    unsigned long long seg_prev = 0;
    bool seg_ev = false;
    // Compiled in by `make profile PFLAGS=-DCRH_DMA_BODY_STAMPS` only: even switched off, the ten tests and the scalars they keep alive
    // lengthen the body the histogram times (the parent's form by a quarter).  Without the flag all of it folds away.
#ifdef CRH_DMA_BODY_STAMPS
    const bool seg_on = a.wave_clock != nullptr && blockIdx.x < 16 && (a.ablate & 32);     // CRH_SCORE_TIMING=2
#else
    constexpr bool seg_on = false;
#endif
    auto seg_stamp = [&](auto Kc) __attribute__((always_inline)) {
        if (seg_on) {
            const unsigned long long t = __builtin_amdgcn_s_memtime();
            seg_tmp[decltype(Kc)::value] = (unsigned)(t - seg_prev);
            seg_prev = t;
        }
    };
#endif
    // M16: the event of user block u at tile ts, in the form the wave's flag selects -- one scalar branch per event
    // (the other forms never take it, but they parse it)
    auto event16 = [&](const AccT& v, float& tau_u, int u, int rows_left, int gi0, unsigned tb, int idv, bool rt) __attribute__((always_inline)) {
        if constexpr (M16) {
            if (lists_full)
                tile_slow_path_dma16<CM, true>(v, tau_u, ls, li, cnt, UB * u, slot0w + UB * u, a, rows_left, gi0, lane, tb, rfilter, idv,
                                               margin, rt CRH_TRIP_ARG);
            else
                tile_slow_path_dma16<CM, false>(v, tau_u, ls, li, cnt, UB * u, slot0w + UB * u, a, rows_left, gi0, lane, tb, rfilter, idv,
                                                margin, rt CRH_TRIP_ARG);
        }
    };
    // body j of the 32x32 forms: MFMAs of tile j (ring slot s_cur) into accumulator set P, threshold test of tile j-1 out of set 1-P;
    // s_nxt = slot of tile j+1, s_fill = slot of tile j + PF (barrier form: the slot tile j-1 left)
    auto body = [&](auto Pc, int j, int s_cur, int s_nxt, int s_fill) __attribute__((always_inline)) {
        // (the 16x16 kernels never call it, but they parse it: what takes the 32x32 accumulators stands under !M16)
        static_assert(!M16 || sizeof(Pc) == 0, "the 16x16 kernels run body16");
        constexpr int P = decltype(Pc)::value, Q = 1 - P;
        const uint32_t src = ring_lds + s_cur * TILE_B, srcn = ring_lds + s_nxt * TILE_B;
        // one group of GR chunks; g is a compile-time constant (every register array below is indexed statically)
        auto group = [&](auto Gc) __attribute__((always_inline)) {
            constexpr int g = decltype(Gc)::value;
            // fragments of the group after next (two groups = 16 MFMAs of slack for the LDS round trip); the last two groups
            // of a tile read the first two of tile j+1, visible since this body's barrier (flag form: since the poll above)
            if constexpr (g + 2 < NG) lds_group(c[(g + 2) & 3], src, std::integral_constant<int, g + 2>{});
            else lds_group(c[(g + 2) & 3], srcn, std::integral_constant<int, g + 2 - NG>{});
            if constexpr (!FL && g == BG) {
                dma_wait_but_newest_tile();             // my pieces of tile j+1 (issued two tiles ago) have landed
                if (!(CRH_ABLATE(a.ablate) & 4)) __builtin_amdgcn_s_barrier();
            }
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (FL) {
                lds_wait_fl(c[g & 3], rflag, dflag);
            } else {
                lds_wait(c[g & 3], std::integral_constant<int, 2 * GR>{});   // this group's fragments (read two groups ago) are in
            }
            // barrier form: tile j+3 into the slot tile j-1 left (every wave is past it); the scheduler places the DMA instructions
            // BETWEEN this group's MFMAs (they follow the wait in program order).  With it the candidate bits of the block
            // of 64 tiles that holds tile j + 32: the current block again (same bytes) in its first half, the NEXT block in
            // its second half -- into the buffer of the block before, whose last tile was selected at the head of body
            // 64 b, before every wave's barrier of that body (flag form: 32 tiles behind every wave, which are at most R apart)
            if constexpr (!FL && g == BG) {
                if constexpr (CM) dma_ids(j + 3);
                else dma_tbits((t0 + j + 32) >> 6);
                dma_tile(j + 3, s_fill);
                // one DMA instruction and a few of its address instructions per MFMA gap instead of all of them in one gap
                // (+0.9 % on the same box: a single wave per SIMD hides about five issue slots per MFMA, not twenty)
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // MFMA
                    __builtin_amdgcn_sched_group_barrier(0x004, 2, 0);   // SALU
                    __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);   // VALU
                    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   // VMEM read (the DMA)
                }
            }
            if constexpr (FL) {
                // The flag protocol, one piece per MFMA gap (n = index of the MFMA just issued, 0 .. 8 UW - 1 in this group):
                //   group 0      n=0  my pieces of tile j + PF - 1 (issued a whole tile ago) have landed -> publish them
                //                n=1  may the slot of tile j + PF - R be refilled?  (poll issued in the last group of the body before)
                //                n=2  the tile bits, n=3 tile j + PF
                //   group NG-3   n=0  poll: is tile j+1 complete?   n=8: the poll has landed, n=9: spin if it is not
                //   group NG-2   n=0  every fragment read of tile j has returned (the group's counted wait left only its own reads
                //                     -- of tile j+1 -- outstanding): the slot may be refilled
                //   group NG-1   n=0  poll for the next body's refill, n=8: landed
                auto hook = [&](auto Nc) __attribute__((always_inline)) {
                    constexpr int n = decltype(Nc)::value;
                    constexpr bool any = (g == 0 && n <= 3) || (g == NG - 3 && (n == 0 || n == 8 || n == 9)) || (g == NG - 2 && n == 0) ||
                                         (g == NG - 1 && (n == 0 || n == 8));
                    if constexpr (any) __builtin_amdgcn_sched_barrier(0);
                    if constexpr (g == 0 && n == 0) {
                        dma_wait_all();
                        flag_bump((j + PF - 1) & (R - 1));
                    }
                    if constexpr (g == 0 && n == 1) flag_spin(dflag, 8 + s_fill, (unsigned)NW * (unsigned)((j + PF) / R));
                    if constexpr (g == 0 && n == 2) dma_tbits((t0 + j + 32) >> 6);
                    if constexpr (g == 0 && n == 3) dma_tile(j + PF, s_fill);
                    if constexpr (g == NG - 3 && n == 0) flag_read(rflag, s_nxt);
                    if constexpr (g == NG - 3 && n == 8) flag_land(rflag);
                    if constexpr (g == NG - 3 && n == 9) flag_spin(rflag, s_nxt, (unsigned)NW * (unsigned)((j + 1) / R + 1));
                    if constexpr (g == NG - 2 && n == 0) flag_bump(8 + s_cur);
                    if constexpr (g == NG - 1 && n == 0) flag_read(dflag, 8 + ((j + 1 + PF) & (R - 1)));
                    if constexpr (g == NG - 1 && n == 8) flag_land(dflag);
                    if constexpr (any) __builtin_amdgcn_sched_barrier(0);
                };
                if constexpr (g == 0) {
#pragma unroll
                    for (int u = 0; u < UW; ++u)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc[P][u][r] = 0.0f;
                }
                if constexpr (sizeof(T) == 4) {
                    [&]<int... JJ>(std::integer_sequence<int, JJ...>) __attribute__((always_inline)) {
                        (mma_f32_hooked<UW, JJ * 4 * UW>(acc[P], c[g & 3][JJ], b[g * GR + JJ], hook), ...);
                    }(std::make_integer_sequence<int, GR>{});
                }
            } else if constexpr (!M16) {
#pragma unroll
                for (int jj = 0; jj < GR; ++jj) {
                    if constexpr (g == 0) {
                        if (jj == 0) {
#pragma unroll
                            for (int u = 0; u < UW; ++u)
#pragma unroll
                                for (int r = 0; r < 16; ++r) acc[P][u][r] = 0.0f;
                        }
                    }
                    Elem<T>::template mma<UW>(acc[P], c[g & 3][jj], b[g * GR + jj]);
                }
            }
            if constexpr (!M16) {
                // the maxima of tile j-1's accumulators: computed and tested in the same group (NU = UW user blocks in the 32x32 forms)
                float m[NU];
                if constexpr (g == TG) {
#pragma unroll
                    for (int u = 0; u < UW; ++u) m[u] = max16(acc[Q][u]);
                }
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (g == TG) {
                    // four compares straight into scalar masks (OR-ed per lane first, the ballot of the result was a select and a second
                    // compare: two VALU instructions per tile beside MFMAs that hide none)
                    unsigned long long hitm = 0ull;
#pragma unroll
                    for (int u = 0; u < UW; ++u) hitm |= __ballot(m[u] > tau[u]);
                    if (hitm != 0ull && live && j > 0 && !(CRH_ABLATE(a.ablate) & 1)) {
#ifdef CRH_PROFILE
                        const unsigned long long ev_t0 = a.wave_clock != nullptr ? __builtin_amdgcn_s_memtime() : 0ull;
#endif
                        const int64_t ts = t0 + j - 1;                                      // the tile being selected
                        const unsigned tb = has_bits ? tbits[((ts >> 6) & 1) * 64 + (ts & 63)] : 0u;
                        int idv = 0;                     // CM: the selected tile's ids, one LDS read per event (where tb's was)
                        if constexpr (CM) idv = (int)tbits[((j - 1) & (IDS_SLOTS - 1)) * 32 + (lane & 31)];
                        // CM: the wave's bit of the tile's rated-tile flags, read with the ids (wave-uniform)
                        bool rt = false;
                        if constexpr (CM) rt = (__builtin_amdgcn_readfirstlane(rtiles[(int)((ts >> 9) & 1) * 64 + (int)((ts >> 3) & 63)]) >> (4 * (int)(ts & 7) + wave)) & 1u;
#pragma unroll
                        for (int u = 0; u < UW; ++u)
                            if (__ballot(m[u] > tau[u]) != 0ull)
                                tile_slow_path_dma<sizeof(T) == 4, CM, MG>(acc[Q][u], tau[u], ls, li, cnt, K, 32 * u, slot0w + 32 * u, a, ts << 5, split_end,
                                                                           lane, tb, rfilter, idv, margin, rt CRH_TRIP_ARG);
                        // the list stores of the inserts are drained HERE: left pending, the compiler parks an lgkmcnt(0) at a
                        // later point of the common path, right behind the fragment reads of the barrier group
                        __builtin_amdgcn_s_waitcnt(0xc07f);
#ifdef CRH_PROFILE
                        if (a.wave_clock != nullptr) {      // CRH_SCORE_TIMING: cycles spent in events and their number, per wave
                            ev_ticks += __builtin_amdgcn_s_memtime() - ev_t0;
                            ev_count += 1;
                        }
#endif
                    }
                }
            }
        };
        [&]<int... Gs>(std::integer_sequence<int, Gs...>) __attribute__((always_inline)) {
            (group(std::integral_constant<int, Gs>{}), ...);
        }(std::make_integer_sequence<int, NG>{});
    };

    // ---- M16: the hand-placed body (round 16).  The same tile as `body` above -- the same 64 MFMAs in the same order, ring, id slots,
    // barrier, DMAs and event -- but every MFMA is followed by ONE slot (hook(g, n), n = the MFMA just issued, fenced by
    // sched_barrier(0)), so what the source puts into a gap stands there in the listing.  A 16-cycle MFMA holds vector issue for 8 of its
    // cycles: a gap hides two 4-cycle vector instructions, or one vector and one or two scalar; a ds_read_b128 or a DMA has a gap to itself.
    //   group 0   gaps 0..15  two of tile j-1's 32 maxima each (user block n >> 1)
    //   group 1   in front: vmcnt, barrier, the counted fragment wait.  gap 0 the tile index, 1 the side-band address, 2 the side-band DMA
    //             (ids, or tile bits), 3 the tile's address, 4 / 5 its two pieces, 8 / 9 the fragment reads of group 3, 10 the ring base
    //   group 2   gaps 0..7 one compare and its s_or each, 8 / 9 the fragment reads of tile j+1's group 0
    //   group 3   gaps 0 / 1 and 6 / 7 the fragment reads of tile j+1's groups 1 and 2
    // The fragment reads are issued in the order g0, g1, g2 (tile j+1), g3 (tile j), two each, every one behind the barrier that publishes
    // its tile and at least 22 MFMAs in front of its group: the counted waits in front of groups 0..3 are lgkmcnt(4), (2), (2), (2).
    // Tile j lives in ring slot j & 3.  ring_a = the LDS base of slot j & 2 of the pair (even tile, odd tile) being multiplied; the odd
    // body moves it on behind its last use, and every other slot is an immediate offset.  Body 0 is peeled (FIRST: no tile in front of
    // it to test, so no `j > 0` in the tail), `live` is folded into the thresholds: the tail is one compare and one branch.
    uint32_t ring_a = ring_lds;
    int next_sync = 0;           // first tile of the next lockstep window (wave 0; beyond the range elsewhere), set in front of the loop
    bool sync_due = false;       // the even body's trip head has a window to report: worked out in a gap of the odd body in front of it
    // Round 22 (BODY_CARRY, the compacted kernel): the fetch of tile j + 3 is state carried from tile to tile and set in front of body 0.
    // A DMA's global address is a scalar base plus a 32-bit lane offset (the saddr form), its LDS slot a scalar byte offset; the barrier
    // group issues the three DMAs from this state and moves it on to tile j + 4 in the gaps behind them.
    //   f_tile   this wave's pieces of the tile (clamped to the stream's last tile, as dma_tile clamps)
    //   f_side   the tile's 32 ids (and the next tile's) in the map
    //   f_soff   per lane, the byte offset of the lane's id from f_side (clamped like dma_ids).  It is worked out a body ahead, in the
    //            gap of piece 1, from
    //   f_sx     the lane clamp the body before that left: 252 bytes, or 124 at the stream's last tile, which has no next tile whose
    //            ids lanes 32 .. 63 could bring
    //   f_ids    LDS byte offset of the ids' slot in tbits;  f_ring  ... of the tile's ring slot
    [[maybe_unused]] const char* f_tile = nullptr;
    [[maybe_unused]] const char* f_side = nullptr;
    [[maybe_unused]] unsigned f_soff = 0, f_sx = 0, f_ids = 0, f_ring = 0;
    [[maybe_unused]] int f_jl = 0;          // body j moves the bases on while j < f_jl: tile t0 + j + 3 is not yet the stream's last
    [[maybe_unused]] unsigned tb_lds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned*)tbits;
    [[maybe_unused]] unsigned lane4 = (unsigned)lane * 4u, lane16 = (unsigned)lane * 16u;
    // BODY_STRAIGHT: what the branch behind a body tests, worked out and pinned in a gap of its group 3.  Behind the odd body: the
    // trip head has something to do or the stream has ended; behind the even body: the stream has ended
    [[maybe_unused]] int trip_rare = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (M16 && BODY_CARRY) {
        asm volatile("" : "+v"(lane4));      // (opaque: one register each for the launch, not a shift per use nor a folded 64-bit pointer;
        asm volatile("" : "+v"(lane16));     // tb_lds: one scalar add per M0, where the symbol's address plus an offset is two)
        asm volatile("" : "+s"(tb_lds));
    }
#endif
    auto lds_wait_bare = [&](auto Nc) __attribute__((always_inline)) {
#if defined(__HIP_DEVICE_COMPILE__)
        if (CRH_ABLATE(a.ablate) & 8) return;    // measurement only: what the fragment waits cost (results invalid)
        // names no register: behind a statement that lists the fragments as outputs hipcc pads the group's first MFMA with an s_nop.
        // The sched_barrier(0) on both sides keeps every MFMA that reads them behind it (cdna_hip_programming.md 5.7: form (iii)).
        // Nothing but that and the register allocator's goodwill keeps a copy or a use of a fragment register from standing between
        // its ds_read_b128 and this wait: tools/body_asm_report.py audits the listing for it (the line "fragment audit"), and the
        // audit is to be repeated whenever hipcc or this body changes
        asm volatile("s_waitcnt lgkmcnt(%0)" ::"i"(decltype(Nc)::value));
#endif
    };
    auto lds_read1 = [&](f32x4& dst, uint32_t addr, auto Oc) __attribute__((always_inline)) {
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(decltype(Oc)::value));
#endif
    };
    auto body16 = [&](auto Pc, auto Fc, int j) __attribute__((always_inline)) {
        constexpr int P = decltype(Pc)::value, Q = 1 - P;
        constexpr bool FIRST = decltype(Fc)::value;
        constexpr int LA = P ? 0 : TILE_B;      // tile j+1 from ring_a: the even body's partner slot, the odd body's moved-on base
        static_assert(CPW == 2 || !M16, "two pieces per wave");
        float m[NU], a0[NU], a1[NU];
        unsigned long long hitm = 0ull;
        unsigned long long hitb[NU];         // the blocks' own masks, kept for the event
        [[maybe_unused]] int tc = 0, tf = 0;
        [[maybe_unused]] const unsigned* side = nullptr;
        [[maybe_unused]] const char* gt = nullptr;
        [[maybe_unused]] unsigned inc = 0, inct = 0;      // BODY_CARRY: steps of the carried state, from gap to gap
        [[maybe_unused]] auto umin = [](unsigned x, unsigned y) __attribute__((always_inline)) { return x < y ? x : y; };
        auto hook = [&](auto Gc, auto Nc) __attribute__((always_inline)) {
            constexpr int g = decltype(Gc)::value, n = decltype(Nc)::value;
            if constexpr (g == 0 && !FIRST) {
#if defined(__HIP_DEVICE_COMPILE__)
                constexpr int u = n >> 1;
                const AccT& v = acc[Q][u];
                if constexpr ((n & 1) == 0) {
                    asm volatile("v_max3_f32 %0, %1, %2, %3" : "=v"(a0[u]) : "v"(v[0]), "v"(v[1]), "v"(v[2]));
                    asm volatile("v_max3_f32 %0, %1, %2, %3" : "=v"(a1[u]) : "v"(v[3]), "v"(v[4]), "v"(v[5]));
                } else {
                    // one statement with one output (round 22).  Between two statements, the second reading what the first wrote, hipcc
                    // puts an s_nop; and behind a statement with a scratch output it puts one too, because it hands the dead scratch
                    // register to the next MFMA's result.  m[u] lives on to group 2: no MFMA of this body is given its register
                    asm volatile("v_max3_f32 %0, %1, %2, %3\n\tv_max_f32 %0, %4, %0"
                                 : "=&v"(m[u])
                                 : "v"(v[6]), "v"(v[7]), "v"(a0[u]), "v"(a1[u]));
                }
#endif
            }
            if constexpr (g == BG && BODY_CARRY) {
#if defined(__HIP_DEVICE_COMPILE__)
                // tile j+3 into the slot tile j-1 left, and its side band, in the issue order of `body`: side band, piece 0, piece 1 -- each
                // out of the carried state, a gap to itself.  (Every step of the state below is pinned to its gap by an empty statement
                // that names the scalar: left alone hipcc sinks all of them to the end of the trip, behind no MFMA.)
                if constexpr (n == 0)
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(f_side + f_soff),
                                                     (__attribute__((address_space(3))) void*)(uintptr_t)(tb_lds + f_ids), 4, 0, 0);
                // (The s_nop between a write of M0 and its DMA stays, twice a tile: the builtin's M0 write is glued to its DMA, so nothing
                // written here can stand between them, and a statement that sets M0 itself would take the register from hipcc.)
                if constexpr (n == 1 || n == 2) {
                    asm volatile("" : "+v"(lane16));      // (opaque in the loop too: a scalar base and this offset, no 64-bit sum per lane)
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(f_tile + lane16),
                                                     (__attribute__((address_space(3))) void*)(ring + f_ring + (wave * CPW) * 1024), 16,
                                                     (n - 1) * 1024, 0);
                }
                if constexpr (n == 2) {
                    f_soff = umin(lane4, f_sx);           // the NEXT body's lane offset, from the clamp the body before left
                    asm volatile("" : "+v"(f_soff));
                }
                // ... and on to tile j+4.  `inc`: the tile just fetched was not the stream's last (the clamp of dma_tile and dma_ids, scalar)
                if constexpr (n == 3) {
                    inc = j < f_jl ? 128u : 0u;                                     // ids: 32 words a tile
                    asm volatile("" : "+s"(inc));
                }
                if constexpr (n == 4) {
                    f_side += inc;
                    asm volatile("" : "+s"(f_side));
                }
                if constexpr (n == 5) {
                    f_sx = j < f_jl - 2 ? 252u : 124u;                              // the clamp of the body after the next: tile t0 + j + 5
                    asm volatile("" : "+s"(f_sx));
                }
                if constexpr (n == 6) {
                    inct = inc << 6;                                                // a tile: TILE_B = 64 * 128 bytes
                    static_assert(TILE_B == 64 * 128 || !M16, "the tile's step is 64 times the ids'");
                    if (CRH_ABLATE(a.ablate) & 2) inct = 0u;
                    asm volatile("" : "+s"(inct));
                }
                if constexpr (n == 7) {
                    f_tile += inct;
                    asm volatile("" : "+s"(f_tile));
                }
                if constexpr (n == 8) lds_read1(c[3][0], ring_a, std::integral_constant<int, P * TILE_B + 3 * 2048>{});
                if constexpr (n == 9) lds_read1(c[3][1], ring_a, std::integral_constant<int, P * TILE_B + 3 * 2048 + 256>{});
                // odd body: that was the pair's last read; the next pair (and this body's look-ahead) starts at slot (j + 1) & 2, two slots
                // from the one just refilled
                if constexpr (n == 10 && P == 1) ring_a = ring_lds + (f_ring ^ (unsigned)(2 * TILE_B));
                if constexpr (n == 11) {
                    f_ids = (f_ids + 128u) & (unsigned)(IDS_SLOTS * 128 - 1);
                    asm volatile("" : "+s"(f_ids));
                }
                if constexpr (n == 12) {
                    f_ring = (f_ring + (unsigned)TILE_B) & (unsigned)(R * TILE_B - 1);
                    asm volatile("" : "+s"(f_ring));
                }
#endif
            }
            if constexpr (g == BG && !BODY_CARRY) {
                // tile j+3 into the slot tile j-1 left, and its side band, in the issue order of `body`: side band, piece 0, piece 1
                if constexpr (n == 0) {
                    tc = (int)t0 + j + 3;
                    tc = tc < n_tiles32 ? tc : n_tiles32 - 1;
                    tf = (CRH_ABLATE(a.ablate) & 2) ? 0 : tc;
                }
                if constexpr (n == 1) {
                    if constexpr (CM) {
                        unsigned e = ((unsigned)tc << 5) + (unsigned)lane;
                        const unsigned e_max = ((unsigned)n_tiles32 << 5) - 1u;
                        e = e < e_max ? e : e_max;
                        side = reinterpret_cast<const unsigned*>(a.idmap) + e;
                    } else {
                        int t = ((int)((t0 + j + 32) >> 6) << 6) + lane;
                        t = t < n_tiles32 ? t : n_tiles32 - 1;
                        side = reinterpret_cast<const unsigned*>(a.tile_bits) + (unsigned)t;
                    }
                }
                if constexpr (n == 2) {
                    unsigned* dst = CM ? tbits + ((j + 3) & (IDS_SLOTS - 1)) * 32 : tbits + (((t0 + j + 32) >> 6) & 1) * 64;
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)side,
                                                     (__attribute__((address_space(3))) void*)dst, 4, 0, 0);
                }
                if constexpr (n == 3) gt = my_pieces + (int64_t)tf * TILE_B;
                if constexpr (n == 4 || n == 5) {
                    char* l = ring + ((j + 3) & (R - 1)) * TILE_B + (wave * CPW) * 1024;
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gt,
                                                     (__attribute__((address_space(3))) void*)l, 16, (n - 4) * 1024, 0);
                }
                if constexpr (n == 8) lds_read1(c[3][0], ring_a, std::integral_constant<int, P * TILE_B + 3 * 2048>{});
                if constexpr (n == 9) lds_read1(c[3][1], ring_a, std::integral_constant<int, P * TILE_B + 3 * 2048 + 256>{});
                // odd body: that was the pair's last read; the next pair (and this body's look-ahead) starts at slot (j + 1) & 2
                if constexpr (n == 10 && P == 1) ring_a = ring_lds + (unsigned)((j + 1) & 2) * TILE_B;
            }
            if constexpr (g == TG) {
                if constexpr (n < NU && !FIRST) {
                    hitb[n] = __ballot(m[n] > tau[n]);
                    hitm |= hitb[n];
                }
                if constexpr (n == 8) lds_read1(c[0][0], ring_a, std::integral_constant<int, LA>{});
                if constexpr (n == 9) lds_read1(c[0][1], ring_a, std::integral_constant<int, LA + 256>{});
            }
            if constexpr (g == 3) {
                if constexpr (n == 0) lds_read1(c[1][0], ring_a, std::integral_constant<int, LA + 2048>{});
                if constexpr (n == 1) lds_read1(c[1][1], ring_a, std::integral_constant<int, LA + 2048 + 256>{});
                if constexpr (n == 6) lds_read1(c[2][0], ring_a, std::integral_constant<int, LA + 2 * 2048>{});
                if constexpr (n == 7) lds_read1(c[2][1], ring_a, std::integral_constant<int, LA + 2 * 2048 + 256>{});
                if constexpr (n == 8 && P == 1) sync_due = (j + 1 >= next_sync) & (j + 1 < n_steps);
                if constexpr (n == 9 && BODY_STRAIGHT && !FIRST) {
                    // the test of the branch behind this body, here and not behind the last MFMA: written out, because hipcc sinks the
                    // C++ form to its use.  Odd body: j + 1 has reached the next window (or rated-tile fetch) or passed the stream's end
#if defined(__HIP_DEVICE_COMPILE__)
                    int rare;
                    if constexpr (P == 1)
                        asm volatile("s_min_i32 %0, %1, %2\n\ts_cmp_ge_i32 %3, %0\n\ts_cselect_b32 %0, 1, 0"
                                     : "=&s"(rare) : "s"(next_sync), "s"(n_steps + 1), "s"(j + 1) : "scc");
                    else
                        asm volatile("s_cmp_gt_i32 %1, %2\n\ts_cselect_b32 %0, 1, 0" : "=s"(rare) : "s"(j + 1), "s"(n_steps) : "scc");
                    trip_rare = rare;
#endif
                }
            }
        };
        auto group = [&](auto Gc) __attribute__((always_inline)) {
            constexpr int g = decltype(Gc)::value;
#ifdef CRH_PROFILE
            // CRH_SCORE_TIMING: the segment that ends here (the front of group 0 ends the group 3 of the body before)
            if constexpr (g == 0) seg_stamp(std::integral_constant<int, 5 * (1 - P) + 4>{});
            else if constexpr (g == BG) seg_stamp(std::integral_constant<int, 5 * P + 0>{});
            else seg_stamp(std::integral_constant<int, 5 * P + g>{});
#endif
            if constexpr (g == BG) {
                dma_wait_but_newest_tile();             // my pieces of tile j+1 (issued two tiles ago) have landed
                if (!(CRH_ABLATE(a.ablate) & 4)) __builtin_amdgcn_s_barrier();
#ifdef CRH_PROFILE
                seg_stamp(std::integral_constant<int, 5 * P + 1>{});
#endif
            }
            __builtin_amdgcn_sched_barrier(0);
            lds_wait_bare(std::integral_constant<int, g == 0 ? 4 : 2>{});
            __builtin_amdgcn_sched_barrier(0);
            [&]<int... N>(std::integer_sequence<int, N...>) __attribute__((always_inline)) {
                (([&]() __attribute__((always_inline)) {
                     constexpr int mb = N >> 3, u = N & 7;
                     AccT& x = acc[P][u];
                     f32x4 t = mb ? f32x4{x[4], x[5], x[6], x[7]} : f32x4{x[0], x[1], x[2], x[3]};
                     if constexpr (g == 0) t = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                     t = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, c[g][mb]), __builtin_bit_cast(f16x8, b[g][u]), t, 0, 0, 0);
#pragma unroll
                     for (int r = 0; r < 4; ++r) x[4 * mb + r] = t[r];
                     __builtin_amdgcn_sched_barrier(0);
                     hook(Gc, std::integral_constant<int, N>{});
                     __builtin_amdgcn_sched_barrier(0);
                 }()),
                 ...);
            }(std::make_integer_sequence<int, 16>{});
            if constexpr (g == TG && !FIRST) {
                // (BODY_STRAIGHT: an event is rare, one tile in 26 at the headline -- its code stands behind the loop's common path)
                if (CRH_DMA_BODY_RARE(BODY_STRAIGHT, hitm != 0ull && !(CRH_ABLATE(a.ablate) & 1))) {
#ifdef CRH_PROFILE
                    const unsigned long long ev_t0 = a.wave_clock != nullptr ? __builtin_amdgcn_s_memtime() : 0ull;
                    seg_ev = true;
#endif
                    const int64_t ts = t0 + j - 1;                                      // the tile being selected
                    const unsigned tb = has_bits ? tbits[((ts >> 6) & 1) * 64 + (ts & 63)] : 0u;
                    int idv = 0;                     // CM: the selected tile's ids, one LDS read per event (where tb's was)
                    if constexpr (CM) idv = (int)tbits[((j - 1) & (IDS_SLOTS - 1)) * 32 + (lane & 31)];
                    // CM: the wave's bit of the tile's rated-tile flags, read with the ids (wave-uniform)
                    bool rt = false;
                    if constexpr (CM) rt = (__builtin_amdgcn_readfirstlane(rtiles[(int)((ts >> 9) & 1) * 64 + (int)((ts >> 3) & 63)]) >> (4 * (int)(ts & 7) + wave)) & 1u;
                    // the rows of the selected tile inside the cut (the clamped last tile of a cut holds fewer than 32) and the id of its
                    // first row, once per event
                    const int64_t rl64 = split_end - (ts << 5);
                    const int rows_left = rl64 < 32 ? (int)rl64 : 32;
                    const int gi0 = (int)(a.item_base + (ts << 5));
#pragma unroll
                    for (int u = 0; u < NU; ++u)
                        // (an event of block u moves tau[u] alone, so the masks of the common path are still those of the blocks behind it)
                        if (hitb[u] != 0ull) event16(acc[Q][u], tau[u], u, rows_left, gi0, tb, idv, rt);
                    // the list stores of the inserts are drained HERE (as in `body`); the fragment reads in flight land with them
                    __builtin_amdgcn_s_waitcnt(0xc07f);
#ifdef CRH_PROFILE
                    if (a.wave_clock != nullptr) {      // CRH_SCORE_TIMING: cycles spent in events and their number, per wave
                        ev_ticks += __builtin_amdgcn_s_memtime() - ev_t0;
                        ev_count += 1;
                    }
#endif
                }
            }
        };
        [&]<int... Gs>(std::integer_sequence<int, Gs...>) __attribute__((always_inline)) {
            (group(std::integral_constant<int, Gs>{}), ...);
        }(std::make_integer_sequence<int, NG>{});
    };

    if (n_steps > 0) {
        if constexpr (CM) {
            dma_ids(0);                                   // tiles 0 .. 3; body j brings tile j + 3 (and j + 4)
            dma_ids(2);
            if (rt_fetch) {                               // the cut's first two blocks, by every wave (identical bytes)
                dma_rtiles(t0 >> 9);
                dma_rtiles((t0 >> 9) + 1);
            } else {
                for (int q = lane; q < RT_B / 4; q += 64) rtiles[q] = a.rated_rowptr != nullptr ? ~0u : 0u;
            }
        } else {
            dma_tbits(t0 >> 6);
            dma_tbits((t0 >> 6) + 1);
        }
#pragma unroll
        for (int p = 0; p < PF; ++p) dma_tile(p, p);
        dma_wait_all();
        __builtin_amdgcn_s_barrier();                     // (also publishes the flag form's initial counters)
        lds_group(c[0], ring_lds, std::integral_constant<int, 0>{});
        lds_group(c[1], ring_lds, std::integral_constant<int, 1>{});
        if constexpr (FL) flag_read(dflag, 8 + (PF & (R - 1)));      // body 0's refill poll (nothing has been read yet: 0 >= 0)
        int s0 = 0;
        // XCD soft lockstep (see xcd_window_sync): wave 0 reports / waits for the workgroup, the others meet it at the
        // tile's barrier
        unsigned* sync_cnt = nullptr;
        int win_steps = 0;
        next_sync = n_steps + 4;
        if (a.xcd_sync && wave == 0) {
            const unsigned xcc = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & 7u;   // HW_REG_XCC_ID
            sync_cnt = a.xcd_sync + (int64_t)xcc * a.sync_stride;
            if (lane == 0) __hip_atomic_fetch_add(sync_cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            win_steps = a.sync_window & ~1;               // whole loop trips (two bodies each)
            if (win_steps < 2) win_steps = 2;
            next_sync = 0;
        }
        // CM: the trip head's rare path serves two clocks, the lockstep windows (next_win) and wave 0's fetch of the next block of
        // rated-tile flags (next_rt); next_sync, which the loop tests, is the earlier of the two.  Block b + 1 is asked for at the first
        // trip head 64 tiles into block b: every wave has passed the barrier of the body before, so the last tile of block b - 1 -- the
        // buffer's old content -- was selected long ago, and the wave's own counted DMA wait of the next body but one publishes the piece
        // at that body's barrier, 440 tiles before its first reader.  Blocks t0 >> 9 and the next one come with the prologue.
        [[maybe_unused]] int next_win = next_sync, next_rt = n_steps + 4;
        if constexpr (CM) {
            if (rt_fetch && wave == 0) next_rt = (int)(((((t0 >> 9) + 1) << 9) + 64) - t0);
            next_sync = next_win < next_rt ? next_win : next_rt;
        }
#ifdef CRH_PROFILE
        unsigned long long t_prev = 0;                  // CRH_SCORE_TIMING: duration of every PAIR of tiles, histogrammed per wave
#endif
        // the head of a loop trip: the CRH_SCORE_TIMING stamp (profile build only) and the lockstep window
        auto trip_head = [&](int j, bool due) __attribute__((always_inline)) {
#ifdef CRH_PROFILE
            if (a.wave_clock != nullptr && blockIdx.x < 16) {
                const unsigned long long t_now = __builtin_amdgcn_s_memtime();
                if (j >= 64 && lane == 0) {
                    // two tiles per trip: 256-cycle units = 128 per tile (fp16); fp32 tiles are 4x as long: 512 per tile
                    unsigned long long dt = (t_now - t_prev) >> ((sizeof(T) == 4 ? 10 : 8) - (ROWB == 256 ? 1 : 0));
                    if (dt > 63) dt = 63;
                    atomicAdd(&a.wave_clock[((size_t)blockIdx.x * 4 + wave) * 64 + dt], 1ull);
                }
                t_prev = t_now;
                // the pair's segments (the hooked 16x16 body stamps them), pairs with an event left out
                if (seg_on && j >= 64 && !seg_ev) {
#pragma unroll
                    for (int q = 0; q < 10; ++q) seg_sum[q] += seg_tmp[q];
                    seg_pairs += 1;
                }
                seg_ev = false;
            }
#endif
            auto window = [&](int& nxt) __attribute__((always_inline)) {
                const int win = j / win_steps;
                if (xcd_window_sync(sync_cnt, win, lane)) {
                    nxt += win_steps;
                } else {                // timed out: run free, and count this workgroup into every window it will not report
                    nxt = n_steps + 4;
                    const int n_win = (n_steps + win_steps - 1) / win_steps;
                    if (lane == 0)
                        for (int wdw = win; wdw < n_win; ++wdw)
                            __hip_atomic_fetch_add(sync_cnt + 1 + wdw, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            };
            if (due) {       // j >= next_sync && j < n_steps: wave 0 only (next_sync stays beyond the range elsewhere)
                if constexpr (CM) {
                    if (j >= next_rt) {
                        dma_rtiles(((t0 + j) >> 9) + 1);
                        next_rt += 512;
                    }
                    if (j >= next_win) window(next_win);
                    next_sync = next_win < next_rt ? next_win : next_rt;
                } else {
                    window(next_sync);
                }
            }
        };
        if constexpr (M16) {
            // body 0 peeled; a trip is then the odd body and the even one behind it, with the trip's head (an even j, as ever) between them
            lds_group(c[2], ring_lds, std::integral_constant<int, 2>{});
            if constexpr (BODY_CARRY) {
                // the carried fetch state for body 0: tile t0 + 3 into ring slot 3, its ids into slot 3
                const int last = n_tiles32 - 1, t3 = (int)t0 + 3;
                const int tc0 = t3 < last ? t3 : last;
                f_jl = last - t3;
                f_tile = packed + (wave * CPW) * 1024 + (int64_t)((CRH_ABLATE(a.ablate) & 2) ? 0 : tc0) * TILE_B;
                f_ring = 3u * (unsigned)TILE_B;
                f_side = reinterpret_cast<const char*>(a.idmap) + (int64_t)tc0 * 128;
                const unsigned lim0 = t3 < last ? 252u : 124u;
                f_soff = lane4 < lim0 ? lane4 : lim0;
                f_sx = t3 + 1 < last ? 252u : 124u;           // body 1's
                f_ids = 3u * 128u;
            }
            trip_head(0, 0 >= next_sync);
            body16(std::integral_constant<int, 0>{}, std::true_type{}, 0);
            for (int j = 1;; j += 2) {                    // (n_steps >= 1: body 1 always runs)
                body16(std::integral_constant<int, 1>{}, std::false_type{}, j);
                if constexpr (BODY_STRAIGHT) {
                    // one test, worked out in the body: a trip falls through odd body, head and even body and takes the back edge alone
                    if (CRH_DMA_BODY_RARE(BODY_STRAIGHT, trip_rare != 0)) {
                        if (j + 1 > n_steps) break;
                        trip_head(j + 1, sync_due);
                    }
#ifdef CRH_PROFILE
                    else trip_head(j + 1, false);             // (its stamp)
#endif
                    body16(std::integral_constant<int, 0>{}, std::false_type{}, j + 1);
                    if (CRH_DMA_BODY_RARE(BODY_STRAIGHT, trip_rare != 0)) break;
                } else {
                    if (j + 1 > n_steps) break;
                    trip_head(j + 1, sync_due);
                    body16(std::integral_constant<int, 0>{}, std::false_type{}, j + 1);
                    if (j + 2 > n_steps) break;
                }
            }
        } else {
            for (int j = 0; j <= n_steps; j += 2) {
                trip_head(j, j >= next_sync && j < n_steps);
                const int s1 = (s0 + 1) & (R - 1), s2 = (s0 + 2) & (R - 1);
                // barrier form: tile j+3 -> slot of tile j-1 = s0 + 3, tile j+4 -> slot of tile j; flag form: tile j + PF -> its own slot
                body(std::integral_constant<int, 0>{}, j, s0, s1, (s0 + PF) & (R - 1));
                if (j + 1 > n_steps) break;
                body(std::integral_constant<int, 1>{}, j + 1, s1, s2, (s1 + PF) & (R - 1));
                s0 = s2;
            }
        }
        dma_wait_all();   // the prefetches of the last bodies must not outlive the workgroup's LDS ...
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(c[0][0]), "+v"(c[0][1]), "+v"(c[1][0]), "+v"(c[1][1]), "+v"(c[2][0]), "+v"(c[2][1]),
                     "+v"(c[3][0]), "+v"(c[3][1]), "+v"(rflag), "+v"(dflag));   // ... nor the last fragment reads / polls their registers
#endif
    }

#ifdef CRH_PROFILE
    if (a.wave_clock != nullptr && blockIdx.x < 16 && lane == 0) {
        a.wave_clock[(size_t)16 * 4 * 64 + ((size_t)blockIdx.x * 4 + wave) * 2] = ev_ticks;
        a.wave_clock[(size_t)16 * 4 * 64 + ((size_t)blockIdx.x * 4 + wave) * 2 + 1] = ev_count;
        a.wave_clock[(size_t)16 * 4 * 66 + ((size_t)blockIdx.x * 4 + wave) * 2] = tp.ticks;
        a.wave_clock[(size_t)16 * 4 * 66 + ((size_t)blockIdx.x * 4 + wave) * 2 + 1] = tp.count;
        // the segments' own region, behind everything the other reports read: [wave][pairs, ten sums]
        a.wave_clock[(size_t)16 * 4 * 68 + ((size_t)blockIdx.x * 4 + wave) * 11] = seg_pairs;
        for (int q = 0; q < 10; ++q) a.wave_clock[(size_t)16 * 4 * 68 + ((size_t)blockIdx.x * 4 + wave) * 11 + 1 + q] = seg_sum[q];
    }
#endif
    if (live) {
        int id_lo, id_hi;
        cut_ids(id_lo, id_hi);
        for (int j = 0; j < UPW; ++j) {
            const int64_t slot = slot0w + j;
            if (slot >= a.n_users) break;
            const int n = __builtin_amdgcn_readfirstlane(cnt[j]);
            const int64_t o = ((int64_t)split * a.n_users + slot) * K;
            if (a.seed_score && S > 1)
                wave_list_store_range(ls + j * K, li + j * K, n, K, a.out_score + o, a.out_idx + o, lane,
                                      split == 0 ? INT32_MIN : id_lo, id_hi);
            else
                wave_list_store(ls + j * K, li + j * K, n, K, a.out_score + o, a.out_idx + o, lane);
        }
    }
}

template <typename T, int D, int R, bool FL, bool CM = false, bool M16 = false>
int launch_score_dma_t(const ScoreArgs& a, hipStream_t stream) {
    const size_t lds = score_dma_lds_bytes(D * (int)sizeof(T), a.k, R, FL, CM);
    auto kern = score_topk_dma_kernel<T, D, R, FL, CM, M16>;
    CRH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds));
    const int64_t blocks = ((a.n_ugroups + DMA_NW - 1) / DMA_NW) * a.n_splits;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(64 * DMA_NW), lds, stream, a);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

}  // namespace

size_t score_dma_lds_bytes(int row_bytes, int k, int ring_slots, bool flags, bool compact) {
    return (size_t)ring_slots * (row_bytes / 32) * 1024 + (compact ? IDS_B + RT_B : TBITS_B) + (flags ? FLAGS_B : 0) + DMA_NW * dma_wave_lds_bytes(k);
}

// Ring slots of a launch, 0 = the lists do not fit beside the ring.  (A flag form with EIGHT slots for 256-byte rows -- prefetch
// distance 5, publish lag 1 -- was built and measured in round 6: at d=64 the per-wave kernel is as fast or faster wherever that
// form beat the barrier form; HISTORY.md, profiles/r06_flag_vs_barrier_vs_wave_ab.log.)
int score_dma_ring_slots(int esz, int d, int k, int mode) {
    const bool fl = esz == 4 && d == 128 && mode == 2;
    return score_dma_lds_bytes(d * esz, k, 4, fl) <= 160 * 1024 ? 4 : 0;
}

// 512-byte rows (fp32 d=128: the headline; fp16 d=256: configs[4]) and 256-byte rows (fp32 d=64: the reference's default
// width, main.py:97 --emb_size 64 = configs[0]; fp16 d=128: the screen of the screened route, score_screen.hip): half the tile,
// half the B registers, the same loop.  mode: 2 = the flag form (fp32 d=128 only), anything else the barrier form.
int launch_score_dma(int esz, int d, int mode, const ScoreArgs& a, hipStream_t stream) {
    // both fp16 d=128 launches are the screen's: their 16x16 form is compiled for its K' and takes no other list length
    if (esz == 2 && d == 128 && a.k != SCREEN_KP) return CRH_ERR_ARG;
    // ... and they carry the margin rule (dma_new_tau): its word and the call's k come with the launch
    if (esz == 2 && d == 128 && (a.margin == nullptr || a.screen_k < 1 || a.screen_k > a.k)) return CRH_ERR_ARG;
    if (esz == 2 && d == 128 && a.idmap != nullptr) {     // the compacted stream of the screened route
        if (score_dma_lds_bytes(d * esz, a.k, 4, false, true) > 160 * 1024) return CRH_ERR_ARG;
        return launch_score_dma_t<_Float16, 128, 4, false, true, true>(a, stream);
    }
    // (fp16 d=128 reaches this kernel from the screen only -- the public fp16 d=128 calls take the ring kernel, score_topk.hip
    // dma_rows -- so both of its launches share one definition of the approximate score)
    if (esz == 2) return d == 128 ? launch_score_dma_t<_Float16, 128, 4, false, false, true>(a, stream) : launch_score_dma_t<_Float16, 256, 4, false>(a, stream);
    if (d == 64) return launch_score_dma_t<float, 64, 4, false>(a, stream);
    return mode == 2 ? launch_score_dma_t<float, 128, 4, true>(a, stream) : launch_score_dma_t<float, 128, 4, false>(a, stream);
}

}  // namespace crh_score
