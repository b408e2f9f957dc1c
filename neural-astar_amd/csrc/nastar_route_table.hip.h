// nastar_route_table.hip.h -- the SUCCESSOR TABLE of a cost-to-go field, one byte per cell, as two families of kernels read it
// (nastar_field_routes.hip.h, item 6i; nastar_path_masks_tiled.hip.h, item 6k): the byte of a cell (frt_cell: fld_best_action on the
// readable field -- the rule is not written here), its two marks and the step an action byte stands for (frt_step).  No kernel lives here,
// so that several translation units may include it.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "nastar_field_rules.hip.h"

namespace nastar {

constexpr uint8_t kRouteNoSucc = 0xFF;  // no successor: not live, or a plateau (kNoSucc of nastar_fields_grad_tiled.hip.h)
constexpr uint8_t kRouteGoal = 0xFE;    // a goal cell: the chase ends here without reading goal[] again

// dy * W + dx of action k: ACTION_MOVES packed two bits per component (value + 1), so that a step is two shifts, two masks and a mad
constexpr uint32_t frt_pack(bool want_dy)
{
    uint32_t v = 0;
    for (int k = 0; k < 8; ++k) v |= (uint32_t)((want_dy ? kActionMoves[k].dy : kActionMoves[k].dx) + 1) << (2 * k);
    return v;
}
__device__ __forceinline__ int frt_step(uint32_t k, int W)
{
    constexpr uint32_t dys = frt_pack(true), dxs = frt_pack(false);
    return ((int)((dys >> (2 * k)) & 3u) - 1) * W + ((int)((dxs >> (2 * k)) & 3u) - 1);
}

// the table byte of cell i of one map
__device__ __forceinline__ uint8_t frt_cell(const float* dist, const float* goal, const float* pass, int i, int H, int W, uint32_t nm)
{
    const float INF = INFINITY;
    if (goal[i] != 0.f) return kRouteGoal;
    const float d = dist[i];
    if (!(d < INF)) return kRouteNoSucc;  // (a NaN is not below +inf)
    const int y = i / W, x = i - y * W;
    auto readable = [&](int dy, int dx) {
        const int j = i + dy * W + dx;
        return pass[j] != 0.f ? dist[j] : INF;
    };
    const int best = fld_best_action(readable, nm, y > 0, y < H - 1, x > 0, x < W - 1, d);
    return best < 0 ? kRouteNoSucc : (uint8_t)best;
}

}  // namespace nastar
