/* nastar_soft_policy.h -- the LOG-POLICY of the entropy-regularised cost-to-go field and the vector-Jacobian product through it, with respect
 * to the cost maps: what a per-cell imitation loss (the cross-entropy between the planner's soft policy and a demonstrated action of every
 * cell) is built on.  An extension BESIDE the other headers: nothing in them changes, NASTAR_VERSION stays what it is -- ask
 * nastar_soft_policy_abi().
 *
 * Moves, the mask, costs, the field V_k, the policy pi_K, "live at k" and the action order are those of nastar_soft_fields.h.  The one-workgroup
 * kernels only: maps of at most nastar_soft_fields_grad_max_cells() cells in the backward, nastar_soft_fields_max_cells() in the forward.
 *
 *   Act(n)      for a cell n live at K: the actions a whose move n -> m_a is in the mask, inside the map, onto a passable cell, with
 *               V_{K-1}(m_a) finite.  Not empty on a live cell.
 *   log-policy  [8,H,W] fp32, the action order of `policy`: logpi_K(a|n) = -(V_{K-1}(m_a) - min) / tau - ln(S), with min and S the soft-min's
 *               minimum and sum at n on plane K-1 -- formed from the two KEPT APART, as the backward forms pi: in the kernel's units of
 *               tau * ln 2 it is ((M - U(m_a)) - log2 S) * ln 2, a difference of two nearby fp32 values, where log(policy) is -inf as soon as a
 *               probability underflows and (V_K(n) - cost[n] - V_{K-1}(m_a)) / tau carries the rounding of |V|.  -inf for an action outside
 *               Act(n); -inf for all eight actions of a cell that is not live at K (a goal, an obstacle, V_K = +inf): the log of the 0 that
 *               `policy` holds there; -inf everywhere on a NASTAR_ERR_BAD_COST map.
 *   forward     nastar_soft_policy_forward writes dist, policy, status and the tape as nastar_soft_cost_to_go does -- the same bits -- and the
 *               log-policy beside them, from the same sweep: no sweep, no plane, no barrier more.  The tape is that call's tape
 *               (nastar_soft_fields_tape_bytes): either forward's tape feeds either backward.
 *
 * The vector-Jacobian product, nastar_soft_policy_backward, with the upstream gradients grad_dist[H,W] (NULL = zeros) and GL[8,H,W] of the
 * log-policy (NULL = zeros):
 *
 *   read        GL(a,n) is read only where n is live at K and a is in Act(n): a NaN or an infinity anywhere else reaches no output (the rule
 *               grad_dist has).
 *   gsum        gsum(n) = the sum over a in Act(n) of GL(a,n), added in the row-major order of the move offsets: (-1,-1) (-1,0) (-1,1) (0,-1)
 *               (0,1) (1,-1) (1,0) (1,1) as (dy, dx).
 *   Z           Z(m) = -(1 / tau) * [the sum over the predecessors n of m that are live at K and step onto m by an allowed move a of
 *               (GL(a,n) - pi_K(a|n) * gsum(n))], gathered at m in the row-major order of the predecessor's position relative to m (the order
 *               of the existing gather), on the cells live at K - 1 and 0 elsewhere: a goal absorbs it.
 *   A           A_{K-1} = (the gather of pi_K * A_K of nastar_soft_fields.h) + Z, in fp32, in that order.  The recurrence k = K-1 .. 1 and the
 *               fp64 sum over k with one rounding at the store are those of nastar_soft_fields_backward, word for word.
 *   K = 1       the log-policy depends on V_0 alone: GL is not read and contributes exactly 0.0f everywhere.
 *   output      linear in the two seeds; exactly 0.0f on a cell that was never live; with GL = NULL the bits of nastar_soft_fields_backward;
 *               with both NULL all zero.  No floating-point atomics: two calls give the same bits.
 *   status      per map, int32: NASTAR_OK, or NASTAR_ERR_BAD_COST (an all-zero grad_cost).
 *
 * No gradient flows to tau.
 */
#ifndef NASTAR_SOFT_POLICY_H_
#define NASTAR_SOFT_POLICY_H_

#include "nastar_soft_fields.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NASTAR_SOFT_POLICY_ABI 1

/* 1: the definition above */
int nastar_soft_policy_abi(void);

/* The arguments of nastar_soft_cost_to_go, and log_policy_out [B,8,H,W] fp32.  One launch on `stream`.  Refused before any HIP call, in this
 * order: an invalid neighbor_mask (NASTAR_ERR_UNSUPPORTED); a NULL cost / goal / passable / dist_out / log_policy_out / status_out
 * (NASTAR_ERR_NULL; policy_out may be NULL: no policy is written); B, H, W or horizon < 1, or a tau that is not finite and positive
 * (NASTAR_ERR_BAD_SHAPE); H*W above nastar_soft_fields_max_cells() (NASTAR_ERR_UNSUPPORTED); a tape that is too small or misaligned
 * (NASTAR_ERR_WORKSPACE). */
int nastar_soft_policy_forward(const float* cost, const float* goal, const float* passable, int B, int H, int W, unsigned neighbor_mask,
                               double tau, int horizon, float* dist_out, float* policy_out, float* log_policy_out, int32_t* status_out,
                               void* tape, size_t tape_bytes, void* stream);

/* The arguments of nastar_soft_fields_backward, with grad_dist [B,H,W] fp32 or NULL (zeros) and grad_log_policy [B,8,H,W] fp32 or NULL
 * (zeros).  One launch on `stream`, nothing is read back.  Refused before any HIP call, in this order: an invalid neighbor_mask
 * (NASTAR_ERR_UNSUPPORTED); a NULL cost / goal / passable / tape / grad_cost_out / status_out (NASTAR_ERR_NULL); B, H, W or horizon < 1, or a
 * tau that is not finite and positive (NASTAR_ERR_BAD_SHAPE); H*W above nastar_soft_fields_grad_max_cells() (NASTAR_ERR_UNSUPPORTED); a tape
 * that is too small or misaligned (NASTAR_ERR_WORKSPACE). */
int nastar_soft_policy_backward(const float* cost, const float* goal, const float* passable, const void* tape, size_t tape_bytes,
                                const float* grad_dist, const float* grad_log_policy, int B, int H, int W, unsigned neighbor_mask, double tau,
                                int horizon, float* grad_cost_out, int32_t* status_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NASTAR_SOFT_POLICY_H_ */
