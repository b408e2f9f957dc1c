// nastar_path_masks_capi.hip -- the C ABI of include/nastar_path_masks.h: the exact shortest path of every map as a 0/1 mask, and its blackbox
// gradient with respect to the costs.  A translation unit of its own: nothing here touches the search, replay, encoder or the other field
// kernels.
#include <hip/hip_runtime.h>

#include <cmath>

#include "nastar_fields_host.hip.h"
#include "nastar_path_masks.hip.h"

using namespace nastar;

// one workgroup per map, the width by the map's size as for nastar_cost_to_go
template <bool kBackward>
static int pmk_launch(const PathMaskArgs& a, int B, hipStream_t s)
{
    const int HW = a.H * a.W;
    const size_t lds = fields_lds_bytes(HW);
    return with_field_block(HW, [&](auto T) { return launch_grid(nastar_path_masks_kernel<T(), kBackward>, dim3((unsigned)B), dim3(T()), lds, s, a); });
}

extern "C" {

int nastar_path_masks_abi(void) { return NASTAR_PATH_MASKS_ABI; }

int nastar_path_masks_max_cells(void) { return kPathMasksMaxCells; }

int nastar_path_masks(const float* cost, const float* goal, const float* passable, const int32_t* start_idx, int B, int H, int W,
                      unsigned neighbor_mask, float* path_out, float* path_cost_out, int32_t* status_out, void* stream)
{
    if (!field_mask_ok(neighbor_mask)) return NASTAR_ERR_UNSUPPORTED;
    if (!cost || !goal || !passable || !start_idx || !path_out || !status_out) return NASTAR_ERR_NULL;
    if (B < 1 || H < 1 || W < 1) return NASTAR_ERR_BAD_SHAPE;
    if ((long long)H * W > kPathMasksMaxCells) return NASTAR_ERR_UNSUPPORTED;  // (the tiled composition is not built into this call)
    const PathMaskArgs a{cost, goal, passable, start_idx, nullptr, nullptr, nullptr, path_out, path_cost_out, status_out, 0.f, 0.f, 0.f, H, W,
                         neighbor_mask, aligned16(cost) && aligned16(goal) && aligned16(passable) ? 1 : 0};
    return pmk_launch<false>(a, B, reinterpret_cast<hipStream_t>(stream));
}

int nastar_path_masks_backward(const float* cost, const float* goal, const float* passable, const int32_t* start_idx,
                               const float* grad_path, const float* path_fwd, const int32_t* status_fwd, int B, int H, int W,
                               unsigned neighbor_mask, float lambda, float min_cost, float* grad_cost_out, int32_t* status_out, void* stream)
{
    if (!field_mask_ok(neighbor_mask)) return NASTAR_ERR_UNSUPPORTED;
    if (!cost || !goal || !passable || !start_idx || !grad_path || !path_fwd || !status_fwd || !grad_cost_out) return NASTAR_ERR_NULL;
    if (B < 1 || H < 1 || W < 1) return NASTAR_ERR_BAD_SHAPE;
    if ((long long)H * W > kPathMasksMaxCells) return NASTAR_ERR_UNSUPPORTED;
    if (!(lambda > 0.f) || !std::isfinite(lambda) || !(min_cost > 0.f) || !std::isfinite(min_cost)) return NASTAR_ERR_UNSUPPORTED;
    const float inv_lambda = 1.0f / lambda;  // one IEEE fp32 division, on the host: what the kernel multiplies by
    if (!std::isfinite(inv_lambda)) return NASTAR_ERR_UNSUPPORTED;  // (a denormal lambda)
    const PathMaskArgs a{cost, goal, passable, start_idx, grad_path, path_fwd, status_fwd, grad_cost_out, nullptr, status_out, lambda, inv_lambda,
                         min_cost, H, W, neighbor_mask,
                         aligned16(cost) && aligned16(goal) && aligned16(passable) && aligned16(grad_path) ? 1 : 0};
    return pmk_launch<true>(a, B, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
