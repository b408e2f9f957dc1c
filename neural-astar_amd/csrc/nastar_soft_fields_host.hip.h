// nastar_soft_fields_host.hip.h -- what the host sides of the one-workgroup soft-field translation units share (nastar_soft_fields_capi.hip,
// nastar_soft_policy_capi.hip): the refusals behind the NULL checks and the choice of the workgroup's width.
#pragma once
#include <cmath>
#include <type_traits>

#include "../../include/nastar_soft_fields.h"
#include "nastar_fields_host.hip.h"

namespace nastar {

// the refusals the entry points share, behind their NULL checks: -> a status, NASTAR_OK to go on
inline int soft_call_ok(int B, int H, int W, double tau, int horizon, int max_cells, const void* tape, size_t tape_bytes)
{
    if (B < 1 || H < 1 || W < 1 || horizon < 1 || !(tau > 0.0) || !std::isfinite(tau)) return NASTAR_ERR_BAD_SHAPE;
    if ((long long)H * W > max_cells) return NASTAR_ERR_UNSUPPORTED;
    if (tape && (tape_bytes < nastar_soft_fields_tape_bytes(B, H, W, horizon) || !aligned16(tape))) return NASTAR_ERR_WORKSPACE;
    return NASTAR_OK;
}

// f(integral_constant<int, T>) for the width T of the workgroup that owns a map of HW cells.  About four cells per lane where the exact
// field takes sixteen (with_field_block): a sweep here is exp2 / log2 issue and, in the backward, a tape read per cell, and what hides
// their latency is wavefronts per CU -- a 32x32 map on ONE wavefront, or a 64x64 backward (100 KiB of LDS: one workgroup per CU) on four,
// ran 2x / 3x slower per cell than the same kernels on sixteen wavefronts per CU.
template <typename F>
int with_soft_block(int HW, F&& f)
{
    if (HW <= 256) return f(std::integral_constant<int, 64>{});
    if (HW <= 1024) return f(std::integral_constant<int, 256>{});
    return f(std::integral_constant<int, 1024>{});
}

}  // namespace nastar
