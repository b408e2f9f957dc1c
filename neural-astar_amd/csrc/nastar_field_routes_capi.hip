// nastar_field_routes_capi.hip -- the C ABI of include/nastar_field_routes.h: ordered optimal routes for many start cells per map, read off
// a cost-to-go field.  A translation unit of its own: nothing here touches the search, replay, encoder or the other field kernels.
#include <hip/hip_runtime.h>

#include "nastar_field_routes.hip.h"
#include "nastar_fields_host.hip.h"

using namespace nastar;

constexpr int kFieldRoutesMaxCells = kTiledMaxCells;
// one byte per cell, and the table is all the LDS the kernel uses: every byte a workgroup may own
constexpr int kFieldRoutesLdsCells = (int)kMaxLdsBytes;
constexpr long long kFieldRoutesMaxQueries = 1ll << 30;
constexpr long long kMaxLanesPerLaunch = 1ll << 31;

static bool frt_shape_ok(int B, int H, int W) { return B >= 1 && H >= 1 && W >= 1 && (long long)H * W <= kFieldRoutesMaxCells; }

// THE DISPATCH between the two homes of the table: up to kFieldRoutesLdsCells cells it lives in LDS
static bool frt_in_lds(int H, int W) { return (long long)H * W <= kFieldRoutesLdsCells; }

// one launch of `kernel` per batch of maps, `groups` workgroups of T lanes per map, at most kMaxLanesPerLaunch lanes per launch
// (groups * T <= S + T or H*W + 4096: one map always fits)
template <typename K>
static int frt_launch(K kernel, FieldRoutesArgs a, int B, long long groups, int T, size_t lds, hipStream_t s)
{
    const long long maps = std::max(1ll, kMaxLanesPerLaunch / T / groups);
    a.groups = (int)groups;
    for (long long b0 = 0; b0 < B; b0 += maps) {
        a.b0 = (int)b0;
        const int rc = launch_grid(kernel, dim3((unsigned)(std::min(maps, B - b0) * groups)), dim3(T), lds, s, a);
        if (rc) return rc;
    }
    return NASTAR_OK;
}

extern "C" {

int nastar_field_routes_abi(void) { return NASTAR_FIELD_ROUTES_ABI; }

int nastar_field_routes_max_cells(void) { return kFieldRoutesMaxCells; }

int nastar_field_routes_lds_cells(void) { return kFieldRoutesLdsCells; }

size_t nastar_field_routes_workspace_bytes(int B, int H, int W)
{
    if (!frt_shape_ok(B, H, W) || frt_in_lds(H, W)) return 0;
    return ((size_t)B * H * W + 15) / 16 * 16;
}

int nastar_field_routes(const float* dist, const float* goal, const float* passable, const int32_t* start_idx, int B, int S, int H, int W,
                        unsigned neighbor_mask, int32_t* routes_out, int route_cap, int32_t* route_len_out, float* route_cost_out,
                        int32_t* status_out, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!field_mask_ok(neighbor_mask)) return NASTAR_ERR_UNSUPPORTED;
    if (!dist || !goal || !passable || !start_idx || !route_len_out || !status_out) return NASTAR_ERR_NULL;
    if (B < 1 || S < 1 || H < 1 || W < 1 || (routes_out && route_cap < 1)) return NASTAR_ERR_BAD_SHAPE;
    if (!frt_shape_ok(B, H, W) || (long long)B * S > kFieldRoutesMaxQueries) return NASTAR_ERR_UNSUPPORTED;
    const size_t need = nastar_field_routes_workspace_bytes(B, H, W);
    if (need && (!workspace || workspace_bytes < need)) return NASTAR_ERR_WORKSPACE;
    const int HW = H * W;
    const bool in_lds = frt_in_lds(H, W);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    FieldRoutesArgs a{dist, goal, passable, start_idx, routes_out, route_len_out, route_cost_out, status_out,
                      in_lds ? nullptr : reinterpret_cast<uint8_t*>(workspace), 0, S, H, W, routes_out ? route_cap : 0, 0, neighbor_mask};
    if (routes_out) {  // every row starts as -1 (0xFF bytes): the kernels store cells only
        hipError_t e = hipMemsetAsync(routes_out, 0xFF, (size_t)B * S * (size_t)route_cap * sizeof(int32_t), s);
        if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(routes_out)");
    }
    if (in_lds)
        return with_field_block(HW, [&](auto T) {
            return frt_launch(nastar_field_routes_lds_kernel<T()>, a, B, ((long long)S + T() - 1) / T(), T(), ((size_t)HW + 15) / 16 * 16, s);
        });
    const int rc = frt_launch(nastar_field_routes_table_kernel, a, B, (HW + kRouteTableCells - 1) / kRouteTableCells, kRouteTableT, 0, s);
    if (rc) return rc;
    return frt_launch(nastar_field_routes_chase_kernel, a, B, ((long long)S + kRouteTableT - 1) / kRouteTableT, kRouteTableT, 0, s);
}

}  // extern "C"
