// nastar_field_routes.hip.h -- ordered optimal routes for many start cells per map, read off a cost-to-go field
// (include/nastar_field_routes.h).
//
// The successor of a cell is fld_best_action on the readable field (nastar_field_rules.hip.h): the rule is not written here.  What is
// here: the SUCCESSOR TABLE, one byte per cell (the action 0..7, kRouteGoal on a goal cell, kRouteNoSucc elsewhere: frt_cell and frt_step
// of nastar_route_table.hip.h, which the tiled path-mask kernels share), its builder
// (frt_build: coalesced loads, the one-cell halo of a cell read from global memory) and the CHASE of one start along it (frt_chase),
// written once and handed the table through an accessor at(n), as the field kernels take at().  Two homes for the table:
//   LDS        nastar_field_routes_lds_kernel<T>: a workgroup of T lanes serves one map and T of its starts; it builds the WHOLE map's
//              table in LDS, and after one barrier each lane chases its start: one ds_read_u8 and a few integer instructions per step.
//              The slices of a map's starts rebuild the table independently: no workgroup waits for another.
//   workspace  nastar_field_routes_table_kernel writes the table (B*H*W bytes), nastar_field_routes_chase_kernel chases it from there,
//              in a second launch.
// A chase that may outgrow its row (route_cap < H*W) runs twice, first for the length, then for the stores; otherwise it stores as it
// goes.  The -1 of the rows are the host's: one memset of routes_out in front of the launch (S lanes per map cannot fill S rows of up
// to H*W entries at the rate of the memory; a memset can).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nastar_field_routes.h"
#include "nastar_field_rules.hip.h"
#include "nastar_route_table.hip.h"

namespace nastar {

constexpr int kRouteTableT = 256;       // the width of the workspace path's two kernels
constexpr int kRouteTableCells = kRouteTableT * kFieldCellsPerLane;  // cells one workgroup of the table kernel writes

struct FieldRoutesArgs {
    const float* dist;       // [B,HW]
    const float* goal;
    const float* passable;
    const int32_t* start;    // [B,S]
    int32_t* routes;         // [B,S,cap] or nullptr
    int32_t* len;            // [B,S]
    float* cost;             // [B,S] or nullptr
    int32_t* status;         // [B,S]
    uint8_t* table;          // [B,HW]: the workspace path's table (nullptr on the LDS path)
    int b0;                  // the first map of this launch
    int S, H, W, cap;
    int groups;              // workgroups per map
    uint32_t nmask;
};

// cells [begin, end) of one map's table, `step` lanes side by side: lane `first` takes begin + first, begin + first + step, ...
__device__ __forceinline__ void frt_build(uint8_t* table, const float* dist, const float* goal, const float* pass, int begin, int end, int first,
                                          int step, int H, int W, uint32_t nm)
{
    for (int i = begin + first; i < end; i += step) table[i] = frt_cell(dist, goal, pass, i, H, W, nm);
}

// THE CHASE of query `row` (= b*S + s) of map `map`, the table behind at(n).  The rows of routes_out hold -1 everywhere when the kernel
// starts (the host's memset): the chase stores the cells it keeps and nothing else.
template <typename At>
__device__ __forceinline__ void frt_chase(const FieldRoutesArgs& a, At at, size_t map, size_t row)
{
    const int HW = a.H * a.W, cap = a.cap;
    const float INF = INFINITY;
    const int n0 = a.start[row];
    const bool inside = n0 >= 0 && n0 < HW;
    const float d0 = inside ? a.dist[map * (size_t)HW + (size_t)n0] : INF;
    int st = !inside ? NASTAR_ERR_BAD_SHAPE : !(fabsf(d0) < INF) ? NASTAR_ERR_UNSOLVABLE : NASTAR_OK;
    int32_t* out = a.routes ? a.routes + row * (size_t)cap : nullptr;
    // visit(n, j) sees the chain's cell j; -> the number of cells, negated for a chain that ends on a cell that is no goal
    auto walk = [&](auto visit) {
        int n = n0, cells = 0;
        uint32_t k = kRouteNoSucc;
        for (int hop = 0; hop < HW; ++hop) {  // the bound: no input moves it (s strictly lowers dist)
            k = at(n);
            visit(n, cells++);
            if (k > 7u) break;
            n += frt_step(k, a.W);
        }
        return k == kRouteGoal ? cells : -cells;
    };
    const bool direct = out && cap >= HW;  // no route outgrows the row: store on the way
    int len = 0;
    if (st == NASTAR_OK) {
        const int cells = walk([&](int n, int j) {
            if (direct) out[j] = n;
        });
        if (cells > 0) {
            len = cells;
            const int skip = len - (len < cap ? len : cap);
            if (out && !direct)
                walk([&](int n, int j) {
                    if (j >= skip) out[j - skip] = n;
                });
        } else {
            st = NASTAR_ERR_PLATEAU;
            if (direct)  // what this lane stored on the way goes, by its own hand: its stores to one address keep their order
                for (int j = 0; j < -cells; ++j) out[j] = -1;
        }
    }
    a.len[row] = len;
    a.status[row] = st;
    if (a.cost) a.cost[row] = d0;
}

// blockIdx.x = (map of this launch) * groups + (slice of the map's starts)
template <int T>
__global__ __launch_bounds__(T) void nastar_field_routes_lds_kernel(const FieldRoutesArgs a)
{
    extern __shared__ uint8_t frt_table[];
    const int tid = threadIdx.x, HW = a.H * a.W;
    const size_t map = (size_t)a.b0 + blockIdx.x / (unsigned)a.groups;
    const int slice = (int)(blockIdx.x % (unsigned)a.groups);
    const size_t base = map * (size_t)HW;
    frt_build(frt_table, a.dist + base, a.goal + base, a.passable + base, 0, HW, tid, T, a.H, a.W, a.nmask);
    __syncthreads();
    const long long s = (long long)slice * T + tid;
    if (s < a.S) frt_chase(a, [&](int n) { return (uint32_t)frt_table[n]; }, map, map * (size_t)a.S + (size_t)s);
}

// blockIdx.x = (map of this launch) * groups + (chunk of kRouteTableCells cells)
__global__ __launch_bounds__(kRouteTableT) void nastar_field_routes_table_kernel(const FieldRoutesArgs a)
{
    const int HW = a.H * a.W;
    const size_t map = (size_t)a.b0 + blockIdx.x / (unsigned)a.groups;
    const int begin = (int)(blockIdx.x % (unsigned)a.groups) * kRouteTableCells;
    const int end = begin + kRouteTableCells < HW ? begin + kRouteTableCells : HW;
    const size_t base = map * (size_t)HW;
    frt_build(a.table + base, a.dist + base, a.goal + base, a.passable + base, begin, end, threadIdx.x, kRouteTableT, a.H, a.W, a.nmask);
}

// behind the table kernel: blockIdx.x = (map of this launch) * groups + (slice of the map's starts)
__global__ __launch_bounds__(kRouteTableT) void nastar_field_routes_chase_kernel(const FieldRoutesArgs a)
{
    const size_t map = (size_t)a.b0 + blockIdx.x / (unsigned)a.groups;
    const long long s = (long long)(blockIdx.x % (unsigned)a.groups) * kRouteTableT + threadIdx.x;
    const uint8_t* table = a.table + map * (size_t)(a.H * a.W);
    if (s < a.S) frt_chase(a, [&](int n) { return (uint32_t)table[n]; }, map, map * (size_t)a.S + (size_t)s);
}

}  // namespace nastar
