// nastar_fields_grad_capi.hip -- the C ABI of include/nastar_fields_grad.h: the gradient of the cost-to-go field with respect to the cost maps.
// A translation unit of its own: nothing here touches the forward field kernels or anything else.
#include <hip/hip_runtime.h>

#include "nastar_fields_grad.hip.h"
#include "nastar_fields_host.hip.h"

using namespace nastar;

static_assert(fields_grad_lds_bytes(kFieldsGradMaxCells) <= kMaxLdsBytes, "A + succ + flags of the largest map fit one workgroup's LDS");
static_assert(kFieldsGradMaxCells == 1024 * kGradCellsPerLane, "the widest workgroup covers the largest map");

extern "C" {

int nastar_fields_grad_abi(void) { return NASTAR_FIELDS_GRAD_ABI; }

int nastar_fields_grad_max_cells(void) { return kFieldsGradMaxCells; }

int nastar_fields_backward(const float* dist, const float* goal, const float* passable, const float* grad_dist, int B, int H, int W,
                           unsigned neighbor_mask, float* grad_cost_out, int32_t* status_out, int32_t* sweeps_out, void* stream)
{
    if (!field_mask_ok(neighbor_mask)) return NASTAR_ERR_UNSUPPORTED;
    if (!dist || !goal || !passable || !grad_dist || !grad_cost_out || !status_out) return NASTAR_ERR_NULL;
    if (B < 1 || H < 1 || W < 1) return NASTAR_ERR_BAD_SHAPE;
    if ((long long)H * W > kFieldsGradMaxCells) return NASTAR_ERR_UNSUPPORTED;
    const int HW = H * W;
    const FieldGradArgs a{dist, goal, passable, grad_dist, grad_cost_out, status_out, sweeps_out, H, W, neighbor_mask};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t lds = fields_grad_lds_bytes(HW);
    return with_field_block(HW, [&](auto T) { return launch_grid(nastar_fields_backward_kernel<T()>, dim3((unsigned)B), dim3(T()), lds, s, a); });
}

}  // extern "C"
