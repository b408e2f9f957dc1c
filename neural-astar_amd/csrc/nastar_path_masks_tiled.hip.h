// nastar_path_masks_tiled.hip.h -- the shortest-path mask of include/nastar_path_masks.h and its blackbox gradient for maps too large for one
// workgroup (include/nastar_path_masks_tiled.h).
//
// The field is nastar_cost_to_go_tiled's, in memory: this file holds what comes in front of that call and behind it.
//   perturb  (backward) w' of every cell, elementwise, with pmk_perturbed of nastar_path_masks.hip.h: the rule is not written again;
//   table    the successor byte of every cell (frt_cell of nastar_route_table.hip.h: fld_best_action on the readable field, the marks for a
//            goal and for a cell without a successor), a workgroup per 4096 cells: what nastar_field_routes chases, in the workspace;
//   mark     one workgroup per map.  (1) all lanes store the row's base value, coalesced: 0, or (0 - path_fwd) * inv_lambda; (2) behind a
//            barrier lane 0 takes the verdict: the start index, the relaxation's per-map status, the field at the start; (3) it chases the
//            start along the table under the unconditional bound of H*W hops -- one byte load and a few integer instructions per step --
//            and stores the route's value on every cell it visits: 1, or (1 - path_fwd) * inv_lambda; (4) a forward chase that ends on a
//            plateau walks again and stores the base value; in the backward every failed map is overwritten with NaN by all lanes behind
//            a second barrier, so that walk is not needed there; (5) status and cost.
// The stores of steps 1, 3 and 4 to one address are ordered by the barriers (steps 1 -> 3, 3 -> NaN) or are one lane's own (3 -> 4).
// Plain vector stores, no atomics, no workgroup waits for another, every output cell is written on every call.
// (A chase that reads the field itself -- goal[] and the eight neighbours' field and passable words of a step loaded together, no table --
// was built first and measured: 0.35 ms slower per call on 512x512 and 1024x1024 maps than the composition with the table, about 250
// instructions per step on one lane against a dozen)
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nastar_path_masks_tiled.h"
#include "nastar_path_masks.hip.h"
#include "nastar_route_table.hip.h"

namespace nastar {

constexpr int kPathMarkT = 1024;   // the row of a map of 1179648 cells: 1152 stores per lane
constexpr int kPerturbT = 256;
constexpr int kPathTableT = 256;
constexpr int kPathTableCells = kPathTableT * kFieldCellsPerLane;  // cells one workgroup of the table kernel writes

struct PathMarkArgs {
    const float* dist;            // [B,HW]: the field as nastar_cost_to_go_tiled left it
    const float* goal;
    const float* passable;
    const int32_t* start;         // [B]
    const int32_t* field_status;  // [B]: the relaxation's verdict
    uint8_t* table;               // [B,HW]: the successor bytes
    const float* path_fwd;        // [B,HW]   (backward)
    const int32_t* status_fwd;    // [B]      (backward)
    float* out;                   // [B,HW]: the mask, or the gradient
    float* path_cost;             // [B] or nullptr (forward)
    int32_t* status;              // [B]; may be nullptr in the backward call
    float inv_lambda;
    int H, W;
    uint32_t nmask;
};

__global__ __launch_bounds__(kPerturbT) void nastar_path_masks_tiled_perturb_kernel(const float* cost, const float* grad_path, float* out,
                                                                                   const size_t cells, const float lambda, const float min_cost)
{
    const size_t stride = (size_t)gridDim.x * kPerturbT;
    for (size_t i = (size_t)blockIdx.x * kPerturbT + threadIdx.x; i < cells; i += stride) out[i] = pmk_perturbed(cost[i], grad_path[i], lambda, min_cost);
}

// blockIdx.x = map * groups + (chunk of kPathTableCells cells)
__global__ __launch_bounds__(kPathTableT) void nastar_path_masks_tiled_table_kernel(const PathMarkArgs a, const int groups)
{
    const int HW = a.H * a.W;
    const size_t map = blockIdx.x / (unsigned)groups;
    const int begin = (int)(blockIdx.x % (unsigned)groups) * kPathTableCells;
    const int end = begin + kPathTableCells < HW ? begin + kPathTableCells : HW;
    const size_t base = map * (size_t)HW;
    for (int i = begin + threadIdx.x; i < end; i += kPathTableT)
        a.table[base + i] = frt_cell(a.dist + base, a.goal + base, a.passable + base, i, a.H, a.W, a.nmask);
}

template <bool kBackward>
__global__ __launch_bounds__(kPathMarkT) void nastar_path_masks_tiled_mark_kernel(const PathMarkArgs a)
{
    __shared__ int verdict;
    const int H = a.H, W = a.W, HW = H * W, tid = threadIdx.x;
    const size_t map = blockIdx.x, base = map * (size_t)HW;
    float* out = a.out + base;
    const float* fwd = kBackward ? a.path_fwd + base : nullptr;
    const float inv_lambda = a.inv_lambda;
    const float INF = INFINITY;

    if constexpr (kBackward) {
        if (a.status_fwd[map] != NASTAR_OK) {  // (the same word for every lane) the forward gave no path: no gradient, the field is not looked at
            for (int i = tid; i < HW; i += kPathMarkT) out[i] = 0.f;
            if (tid == 0 && a.status) a.status[map] = NASTAR_OK;
            return;
        }
    }

    // ---- (1) the base value of the row -------------------------------------------------------------------------------------------------------------
    auto value = [&](int i, float y) { return kBackward ? (y - fwd[i]) * inv_lambda : y; };
    for (int i = tid; i < HW; i += kPathMarkT) out[i] = value(i, 0.f);
    __syncthreads();

    if (tid == 0) {
        // ---- (2) the verdict, in the header's order ------------------------------------------------------------------------------------------------
        const float* D = a.dist + base;
        const uint8_t* table = a.table + base;
        const int n0 = a.start[map];
        int st = !(n0 >= 0 && n0 < HW) ? NASTAR_ERR_BAD_SHAPE : a.field_status[map];   // 9, 3 (no goal) or 10
        float d0 = INF;
        if (st == NASTAR_OK) {
            d0 = D[n0];
            if (!(d0 < INF)) st = NASTAR_ERR_UNSOLVABLE;
        }
        if (st == NASTAR_OK) {
            // ---- (3) the chase: visit(n) sees every cell of the chain; -> it ended on a goal ------------------------------------------------------------
            auto walk = [&](auto visit) {
                int n = n0;
                uint32_t k = kRouteNoSucc;
                for (int hop = 0; hop < HW; ++hop) {  // the bound: no input moves it (s strictly lowers the field)
                    k = table[n];
                    visit(n);
                    if (k > 7u) break;
                    n += frt_step(k, W);
                }
                return k == kRouteGoal;
            };
            if (!walk([&](int n) { out[n] = value(n, 1.f); })) {
                st = NASTAR_ERR_PLATEAU;
                // ---- (4) the marks go, by the hand that made them ----------------------------------------------------------------------------------------
                if constexpr (!kBackward) walk([&](int n) { out[n] = 0.f; });
            }
        }
        // ---- (5) ---------------------------------------------------------------------------------------------------------------------------------------
        if (a.status) a.status[map] = st;
        if (!kBackward && a.path_cost) a.path_cost[map] = st == NASTAR_OK ? d0 : INF;
        verdict = st;
    }
    if constexpr (kBackward) {
        __syncthreads();
        if (verdict != NASTAR_OK)  // the perturbed solve failed: a loud row
            for (int i = tid; i < HW; i += kPathMarkT) out[i] = NAN;
    }
}

}  // namespace nastar
