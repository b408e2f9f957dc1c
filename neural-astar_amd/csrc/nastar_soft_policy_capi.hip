// nastar_soft_policy_capi.hip -- the C ABI of include/nastar_soft_policy.h: the log-policy of the entropy-regularised cost-to-go field and the
// gradient through it.  A translation unit of its own: the kernels of nastar_soft_fields_capi.hip are not touched.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "nastar_soft_fields_host.hip.h"
#include "nastar_soft_policy.hip.h"

using namespace nastar;

extern "C" {

int nastar_soft_policy_abi(void) { return NASTAR_SOFT_POLICY_ABI; }

int nastar_soft_policy_forward(const float* cost, const float* goal, const float* passable, int B, int H, int W, unsigned neighbor_mask,
                               double tau, int horizon, float* dist_out, float* policy_out, float* log_policy_out, int32_t* status_out,
                               void* tape, size_t tape_bytes, void* stream)
{
    if (!field_mask_ok(neighbor_mask)) return NASTAR_ERR_UNSUPPORTED;
    if (!cost || !goal || !passable || !dist_out || !log_policy_out || !status_out) return NASTAR_ERR_NULL;
    if (int rc = soft_call_ok(B, H, W, tau, horizon, kSoftFieldsMaxCells, tape, tape_bytes)) return rc;
    const int HW = H * W;
    const double unit = tau * M_LN2;
    const SoftFieldArgs a{cost, goal, passable, dist_out, policy_out, status_out, static_cast<float*>(tape), H, W, horizon, neighbor_mask,
                          (float)(1.0 / unit), (float)unit};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t lds = soft_fields_lds_bytes(HW);
    return with_soft_block(HW, [&](auto T) {
        return launch_grid(nastar_soft_policy_forward_kernel<T()>, dim3((unsigned)B), dim3(T()), lds, s, a, log_policy_out);
    });
}

int nastar_soft_policy_backward(const float* cost, const float* goal, const float* passable, const void* tape, size_t tape_bytes,
                                const float* grad_dist, const float* grad_log_policy, int B, int H, int W, unsigned neighbor_mask, double tau,
                                int horizon, float* grad_cost_out, int32_t* status_out, void* stream)
{
    if (!field_mask_ok(neighbor_mask)) return NASTAR_ERR_UNSUPPORTED;
    if (!cost || !goal || !passable || !tape || !grad_cost_out || !status_out) return NASTAR_ERR_NULL;
    if (int rc = soft_call_ok(B, H, W, tau, horizon, kSoftFieldsGradMaxCells, tape, tape_bytes)) return rc;
    const int HW = H * W;
    // (the tape is in units of tau * ln 2 and the field's gradient needs no factor; the log-policy is a plane's difference OVER tau)
    const SoftFieldGradArgs a{cost, goal, passable, static_cast<const float*>(tape), grad_dist, grad_cost_out, status_out, H, W, horizon, neighbor_mask};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t lds = soft_fields_grad_lds_bytes(HW);
    return with_soft_block(HW, [&](auto T) {
        return launch_grid(nastar_soft_policy_backward_kernel<T()>, dim3((unsigned)B), dim3(T()), lds, s, a, grad_log_policy, (float)(-1.0 / tau));
    });
}

}  // extern "C"
