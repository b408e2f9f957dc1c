// nastar_fields_capi.hip -- the C ABI of include/nastar_fields.h: the cost-to-go field of whole maps and its optimal policy.  A translation
// unit of its own: nothing here touches the search, replay or encoder kernels.
#include <hip/hip_runtime.h>

#include "nastar_fields.hip.h"
#include "nastar_fields_host.hip.h"

using namespace nastar;

extern "C" {

int nastar_fields_abi(void) { return NASTAR_FIELDS_ABI; }

int nastar_fields_max_cells(void) { return kFieldsMaxCells; }

int nastar_cost_to_go_sweeps(const float* cost, const float* goal, const float* passable, int B, int H, int W, unsigned neighbor_mask,
                             float* dist_out, float* policy_out, int32_t* status_out, int32_t* sweeps_out, void* stream)
{
    if (!field_mask_ok(neighbor_mask)) return NASTAR_ERR_UNSUPPORTED;
    if (!cost || !goal || !passable || !dist_out || !status_out) return NASTAR_ERR_NULL;
    if (B < 1 || H < 1 || W < 1) return NASTAR_ERR_BAD_SHAPE;
    if ((long long)H * W > kFieldsMaxCells) return NASTAR_ERR_UNSUPPORTED;
    const int HW = H * W;
    const FieldArgs a{cost, goal, passable, dist_out, policy_out, status_out, sweeps_out, H, W, neighbor_mask,
                      aligned16(cost) && aligned16(goal) && aligned16(passable) ? 1 : 0};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t lds = fields_lds_bytes(HW);
    return with_field_block(HW, [&](auto T) { return launch_grid(nastar_cost_to_go_kernel<T()>, dim3((unsigned)B), dim3(T()), lds, s, a); });
}

int nastar_cost_to_go(const float* cost, const float* goal, const float* passable, int B, int H, int W, unsigned neighbor_mask, float* dist_out,
                      float* policy_out, int32_t* status_out, void* stream)
{
    return nastar_cost_to_go_sweeps(cost, goal, passable, B, H, W, neighbor_mask, dist_out, policy_out, status_out, nullptr, stream);
}

}  // extern "C"
