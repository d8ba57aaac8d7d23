// The reverse index of one BPR batch ("plan"): its memory layout, in this file and nowhere else.
//
// A plan is int32, built on the device (bpr_plan.hip) or on the host next to the sampler (crh_bpr_plan_build_host):
//   [0] nu  [1] ni  [2] L = layout batch size (>= the batch; one stride for all batches of an epoch)
//   [3 .. 3+L)  user rows touched (ascending), then (L+1) offsets into the user list, L triple ids
//   grouped by user row; then 2L item rows, (2L+1) offsets, 2L entries  b | (role << 30)
//   (role 0 = positive, 1 = negative); then [n_heavy, heavy row slots...] (see plan_heavy_off).
// One lane group owns one touched row and sums its contributions in list order, then STORES the
// row of the dense gradient table (which is zero everywhere else): no atomics, bit-reproducible.
// The plan ends with the list of HEAVY rows (more than BPR_HEAVY entries): [n_heavy, slot, slot, ...] where a slot
// is the row's position w in the concatenated (user rows, item rows) list, ascending; at most 3L/(BPR_HEAVY+1) of them.
//
// Readers: the plan backward and the row exchange (bpr.hip), the touched-rows optimisers (optim.hip), the one-launch MF
// step and its per-epoch tables (mf_step.hip).  Writers: bpr_plan.hip.
#pragma once
#include "crh_common.h"

// entries of one gradient row above which a whole block sums it: a lane group walks a row's list sequentially (one
// round trip per 4 entries), so the longest "light" row sets the kernel's critical path -- 8 keeps it at two trips.
// One-launch MF step, us per step at the MovieLens shape: 8 (with 96 heavy blocks) 18.0, 4 28.6, 6 19.7, 12 19.6
// (HISTORY.md section 4.3, the round-3 re-check).
constexpr int BPR_HEAVY = 8;

__host__ __device__ inline int64_t plan_heavy_cap(int64_t L) { return 3 * L / BPR_HEAVY + 2; }
__host__ __device__ inline int64_t plan_heavy_off(int64_t L) { return 3 + (3 * L + 1) + (6 * L + 1); }
__host__ __device__ inline int64_t plan_ints(int64_t L) { return plan_heavy_off(L) + 1 + plan_heavy_cap(L); }
// entries of one batch: the L of its user list, then the 2L of its item list (the order mf_step.hip's tables keep)
__host__ __device__ inline int64_t plan_entries(int64_t L) { return 3 * L; }

// The seven sections of a plan behind its three header ints; T = int32_t (builders) or const int32_t (readers).
// `heavy` is the heavy section's first int, the count; the slots follow it.
template <typename T>
struct PlanSections {
    T *urow, *uptr, *ulist, *irow, *iptr, *ilist, *heavy;
};

template <typename T>
__host__ __device__ __forceinline__ PlanSections<T> plan_sections(T* pl, int64_t L) {
    PlanSections<T> s;
    s.urow = pl + 3;
    s.uptr = s.urow + L;
    s.ulist = s.uptr + (L + 1);
    s.irow = s.ulist + L;
    s.iptr = s.irow + 2 * L;
    s.ilist = s.iptr + (2 * L + 1);
    s.heavy = pl + plan_heavy_off(L);
    return s;
}

// A finished plan as its readers see it: the sections plus the header ints; heavy[1 + h] is the h-th heavy slot.
struct PlanView : PlanSections<const int32_t> {
    int n_u, n_i, n_heavy;
};

__device__ __forceinline__ PlanView plan_view(const int32_t* pl) {
    PlanView v{plan_sections(pl, pl[2])};
    v.n_u = pl[0];
    v.n_i = pl[1];
    v.n_heavy = v.heavy[0];
    return v;
}

// is slot r of the concatenated (user rows, item rows) list a heavy row?
__host__ __device__ __forceinline__ int plan_row_heavy(const int32_t* uptr, const int32_t* iptr, int nu, int r) {
    return (r < nu ? uptr[r + 1] - uptr[r] : iptr[r - nu + 1] - iptr[r - nu]) > BPR_HEAVY;
}
