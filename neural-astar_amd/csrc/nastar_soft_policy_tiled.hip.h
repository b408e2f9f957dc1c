// nastar_soft_policy_tiled.hip.h -- the LOG-POLICY of the tiled entropy-regularised cost-to-go field and its adjoint
// (include/nastar_soft_policy_tiled.h): the other side of the compile-time switches of the kernels in
// nastar_soft_fields_tiled.hip.h, as nastar_soft_policy.hip.h is of the one-workgroup bodies.
//
// FORWARD.  nastar_soft_tiled_sweeps_kernel<T, true>: the launch that reaches plane K holds plane K-1 on its tile and one ring; its
// epilogue writes logpi_K(a|n) = ((M - U(m_a)) - log2 S) ln 2 beside pi_K(a|n) = exp2(M - U(m_a)) / S, from the same M and S -- the
// expression of sfl_forward<T, true>, operand for operand.  No sweep, no plane and no launch more; the launches below K are the plain
// kernel's.
//
// BACKWARD.  nastar_soft_tiled_grad_step_kernel<T, true>, launched for step K only: the first pass, on the tile and one ring, also forms
// Q(n) = gsum(n) / S_K(n) where n is live at K -- "live at K" read from C and plane K (the tape's final slot), as the init kernel reads it,
// never re-derived from the soft-min -- and the gather adds z += GL(a,n) - w Q(n) over the predecessors live at K:
// A_{K-1} = acc + z * (-1 / tau).  Q and the live bytes stay in LDS (soft_tile_inject_lds_bytes); GL is read from device memory, at n for
// gsum and at the predecessor in the gather (the second read is the L2's).  One workgroup owns a cell: no atomics.
#pragma once
#include "../../include/nastar_soft_policy_tiled.h"
#include "nastar_soft_fields_tiled.hip.h"
#include "nastar_soft_policy.hip.h"  // (sfp_offsets_mirror: kOppositeAction[7 - j] is the action whose move is kChildOffsets[j])

namespace nastar {

// the three instantiations of this side of the switches, under the names the host side launches them by
template <int T>
constexpr auto nastar_soft_policy_tiled_sweeps_kernel = &nastar_soft_tiled_sweeps_kernel<T, true>;          // (a, log_policy)
template <int T>
constexpr auto nastar_soft_policy_tiled_grad_init_kernel = &nastar_soft_tiled_grad_init_kernel<T, true>;    // a.grad_dist may be nullptr (zeros)
template <int T>
constexpr auto nastar_soft_policy_tiled_inject_step_kernel = &nastar_soft_tiled_grad_step_kernel<T, true>;  // a.U is plane K - 1, seed.UK plane K

}  // namespace nastar
