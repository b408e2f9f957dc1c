// nastar_routes.hip.h -- ordered routes out of the search launch (include/nastar_routes.h): the parent chain that `backtrack` marks, in
// travel order, its length and its cost, written by the epilogue of every search kernel when the launch carries a `routes_out` pointer.
// The pointer is null for every entry point of include/nastar.h: their kernels test it once (wave-uniform) and do nothing else here.
//
// Per map b:
//   route      the goal, then the hops the backtrack walk takes from the goal's parent (at most `walk_cap`, ending at the start or at a
//              cell that was never opened), reversed: the goal comes LAST.  Empty for a map without a one-hot goal or whose search was refused.
//   len[b]     number of route cells -- the true length, also when the row is shorter
//   row[b, :]  `cap` int32: the last min(len, cap) cells of the route (flat indices r*W + c; the goal at min(len, cap) - 1), then -1 to the end
//   cost[b]    fp32(sum in fp64 of the cost of every route cell but the goal): the costs of the cells being LEFT, what the search's g adds up
//
// Shape: lane 0 walks the chain twice.  Walk 1 counts the cells and sums their costs; walk 2 stores cell k hops from the goal at
// row[min(len, cap) - 1 - k] -- fire-and-forget 4-byte stores, nothing is read back, so no memory ordering is involved.  All 64 lanes
// then fill the tail with coalesced stores.  One LDS (large-map kernel: slab) round trip per hop and walk, only when routes are asked for.
#pragma once
#include "nastar_search.hip.h"

namespace nastar {

// the optional route outputs of a forward launch, as the kernels' argument structs carry them (all null / 0 unless the entry point is
// nastar_forward_routes / nastar_forward_routes_batchloop_finish)
struct RouteOut {
    int* routes = nullptr;  // [B][cap]
    int cap = 0;
    int* len = nullptr;     // [B]
    float* cost = nullptr;  // [B], optional
};

// The route group of the running kernel, read from its argument segment WHERE IT IS USED (the epilogue).  Read as ordinary members of the
// argument struct, the four values are loaded at kernel entry and held in scalar registers through the step loop: 7 more SGPRs, which
// took one wavefront per SIMD from the large-map kernel and the runtime-size compiled loops (102 instead of 96) and made the unit-cost
// kernel spill.  kOffset = offsetof(<argument struct>, route); the struct is the kernel's FIRST parameter (it starts the segment).
template <size_t kOffset>
__device__ __forceinline__ RouteOut kernel_route_args()
{
    typedef const RouteOut __attribute__((address_space(4))) * SegPtr;
    uint64_t seg = (uint64_t)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(seg));  // opaque from here on: the loads below stay behind the step loop
    const SegPtr p = (SegPtr)(seg + kOffset);
    RouteOut r;
    r.routes = p->routes;
    r.cap = p->cap;
    r.len = p->len;
    r.cost = p->cost;
    return r;
}

// pdir: the map's parent codes (LDS or the HBM slab; the backtrack walk has run).  parent_of(cell, code) -> the parent cell;
// cost_of(cell) -> fp32 cost of a route cell.  has_route: the map has a one-hot goal and was searched (else: the empty route).
// walk_cap: the backtrack walk's own cap.  Returns min(len, cap) (wave-uniform): the caller fills row[that .. cap) with -1.
template <typename ParentOf, typename CostOf>
__device__ __forceinline__ int route_walk(const uint8_t* pdir, int lane, int start_idx, int goal_idx, int walk_cap, bool has_route,
                                          ParentOf parent_of, CostOf cost_of, const RouteOut& ro, int b)
{
    int n = 0;
    if (lane == 0) {
        int len = 0;
        double sum = 0.0;
        int* const row = ro.routes + (size_t)b * (size_t)ro.cap;
        if (has_route) {
            const uint32_t code = pdir[goal_idx] & P_DIRMASK;
            const int first = code != PARENT_UNSET ? parent_of(goal_idx, code) : -1;
            len = 1;
            if (first >= 0) {
                int loc = first;
                for (int k = 0; k < walk_cap; ++k) {  // the walk of backtrack, hop for hop
                    if (loc == goal_idx) break;  // (lock-step mode expands the goal: a chain that returns to it marks nothing new)
                    ++len;
                    sum += (double)cost_of(loc);
                    if (loc == start_idx) break;
                    const uint32_t cd = pdir[loc] & P_DIRMASK;
                    if (cd == PARENT_UNSET) break;
                    loc = parent_of(loc, cd);
                }
            }
            n = len < ro.cap ? len : ro.cap;
            row[n - 1] = goal_idx;
            int loc = first;
            for (int k = 1; k < n; ++k) {  // (k < len: `loc` is a cell walk 1 visited, and every one before the last has a parent)
                row[n - 1 - k] = loc;
                if (k + 1 < n) loc = parent_of(loc, pdir[loc] & P_DIRMASK);
            }
        }
        ro.len[b] = len;
        if (ro.cost != nullptr) ro.cost[b] = (float)sum;
    }
    return __builtin_amdgcn_readfirstlane(n);
}

// row[from .. cap) = -1, all 64 lanes
__device__ __forceinline__ void route_fill_tail(const RouteOut& ro, int b, int from, int lane)
{
    int* const row = ro.routes + (size_t)b * (size_t)ro.cap;
    for (int i = from + lane; i < ro.cap; i += 64) row[i] = -1;
}

}  // namespace nastar
