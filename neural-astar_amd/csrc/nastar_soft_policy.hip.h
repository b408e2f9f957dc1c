// nastar_soft_policy.hip.h -- the LOG-POLICY of the entropy-regularised cost-to-go field and its adjoint (include/nastar_soft_policy.h;
// DESIGN.md section 2, item 6n): the other side of the compile-time switch of the two bodies in nastar_soft_fields.hip.h.
//
// FORWARD.  sfl_forward<T, true>: the epilogue that writes pi_K(a|n) = exp2(M - U(m_a)) / S also writes
// logpi_K(a|n) = ((M - U(m_a)) - log2 S) ln 2 from the same M, S and plane K-1 in LDS -- no sweep, no plane and no barrier more; dist, policy,
// status and the tape are the statements, and so the bits, of nastar_soft_cost_to_go_kernel.
//
// BACKWARD.  sfl_backward<T, true>: with d logpi_K(a|n) / d V_{K-1}(m_b) = -(1 / tau) ([a = b] - pi_K(b|n)), the seed GL reaches plane K-1 as
//   Z(m) = -(1 / tau) * sum over the predecessors n of m live at K of (GL(a,n) - pi_K(a|n) gsum(n)),   gsum(n) = sum over Act(n) of GL(., n),
// added to the gather of step K; the steps K-1 .. 1 are the plain ones.  The 25 B per cell of the plain backward fill the LDS at 6144 cells, so
// the one fp32 per cell the injection needs, Q(n) = gsum(n) / S_K(n), borrows the fp64 sum's slot for that step (sfl_backward says how).  GL is
// read from global memory, at n for gsum and at m in the gather (the second read is the L2's), on the entries (live at K, Act) only.
#pragma once
#include "../../include/nastar_soft_policy.h"
#include "nastar_soft_fields.hip.h"

namespace nastar {

// kChildOffsets mirrors about its middle, so the action of the MOVE kChildOffsets[j] is kOppositeAction[7 - j] (what sfl_backward's gsum reads)
constexpr bool sfp_offsets_mirror()
{
    for (int j = 0; j < 8; ++j)
        if (kChildOffsets[7 - j].dy != -kChildOffsets[j].dy || kChildOffsets[7 - j].dx != -kChildOffsets[j].dx) return false;
    return true;
}
static_assert(sfp_offsets_mirror(), "kOppositeAction[7 - j] is the action whose move is kChildOffsets[j]");

template <int T>
__global__ __launch_bounds__(T) void nastar_soft_policy_forward_kernel(const SoftFieldArgs a, float* log_policy)
{
    sfl_forward<T, true>(a, log_policy);
}

// grad_log_policy: [B,8,HW] or nullptr; a.grad_dist may be nullptr too
template <int T>
__global__ __launch_bounds__(T) void nastar_soft_policy_backward_kernel(const SoftFieldGradArgs a, const float* grad_log_policy, float neg_inv_tau)
{
    const float* gl = grad_log_policy ? grad_log_policy + (size_t)blockIdx.x * 8 * a.H * a.W : nullptr;
    sfl_backward<T, true>(a, SoftPolicySeed{gl, neg_inv_tau});
}

}  // namespace nastar
