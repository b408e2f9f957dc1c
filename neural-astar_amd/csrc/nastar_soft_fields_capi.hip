// nastar_soft_fields_capi.hip -- the C ABI of include/nastar_soft_fields.h: the entropy-regularised cost-to-go field over a finite horizon and
// its gradient with respect to the cost maps.  A translation unit of its own: nothing here touches the other field kernels.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "nastar_soft_fields.hip.h"
#include "nastar_soft_fields_host.hip.h"

using namespace nastar;

static_assert(soft_fields_lds_bytes(kSoftFieldsMaxCells) <= kMaxLdsBytes, "C + two planes + flags of the largest map fit one workgroup's LDS");
static_assert(soft_fields_grad_lds_bytes(kSoftFieldsGradMaxCells) <= kMaxLdsBytes, "the backward's planes of its largest map fit too");
static_assert(kSoftFieldsGradMaxCells <= kSoftFieldsMaxCells, "what the backward takes, the forward takes");

extern "C" {

int nastar_soft_fields_abi(void) { return NASTAR_SOFT_FIELDS_ABI; }

int nastar_soft_fields_max_cells(void) { return kSoftFieldsMaxCells; }

int nastar_soft_fields_grad_max_cells(void) { return kSoftFieldsGradMaxCells; }

size_t nastar_soft_fields_tape_bytes(int B, int H, int W, int horizon)
{
    if (B < 1 || H < 1 || W < 1 || horizon < 1) return 0;
    const unsigned __int128 n = (unsigned __int128)B * (unsigned)horizon * ((unsigned __int128)H * (unsigned)W) * 4u;
    return n > (unsigned __int128)SIZE_MAX ? SIZE_MAX : (size_t)n;
}

int nastar_soft_cost_to_go(const float* cost, const float* goal, const float* passable, int B, int H, int W, unsigned neighbor_mask, double tau,
                           int horizon, float* dist_out, float* policy_out, int32_t* status_out, void* tape, size_t tape_bytes, void* stream)
{
    if (!field_mask_ok(neighbor_mask)) return NASTAR_ERR_UNSUPPORTED;
    if (!cost || !goal || !passable || !dist_out || !status_out) return NASTAR_ERR_NULL;
    if (int rc = soft_call_ok(B, H, W, tau, horizon, kSoftFieldsMaxCells, tape, tape_bytes)) return rc;
    const int HW = H * W;
    const double unit = tau * M_LN2;
    const SoftFieldArgs a{cost, goal, passable, dist_out, policy_out, status_out, static_cast<float*>(tape), H, W, horizon, neighbor_mask,
                          (float)(1.0 / unit), (float)unit};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t lds = soft_fields_lds_bytes(HW);
    return with_soft_block(HW, [&](auto T) { return launch_grid(nastar_soft_cost_to_go_kernel<T()>, dim3((unsigned)B), dim3(T()), lds, s, a); });
}

int nastar_soft_fields_backward(const float* cost, const float* goal, const float* passable, const void* tape, size_t tape_bytes,
                                const float* grad_dist, int B, int H, int W, unsigned neighbor_mask, double tau, int horizon,
                                float* grad_cost_out, int32_t* status_out, void* stream)
{
    if (!field_mask_ok(neighbor_mask)) return NASTAR_ERR_UNSUPPORTED;
    if (!cost || !goal || !passable || !tape || !grad_dist || !grad_cost_out || !status_out) return NASTAR_ERR_NULL;
    if (int rc = soft_call_ok(B, H, W, tau, horizon, kSoftFieldsGradMaxCells, tape, tape_bytes)) return rc;
    const int HW = H * W;
    // (the tape is kept in units of tau * ln 2 and the gradient with respect to the cost needs no factor: tau is checked and not used)
    const SoftFieldGradArgs a{cost, goal, passable, static_cast<const float*>(tape), grad_dist, grad_cost_out, status_out, H, W, horizon, neighbor_mask};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t lds = soft_fields_grad_lds_bytes(HW);
    return with_soft_block(HW, [&](auto T) { return launch_grid(nastar_soft_fields_backward_kernel<T()>, dim3((unsigned)B), dim3(T()), lds, s, a); });
}

}  // extern "C"
