/* nastar_soft_fields.h -- the ENTROPY-REGULARISED (soft-min) cost-to-go field of whole maps over a finite horizon, its soft policy, and the
 * vector-Jacobian product with respect to the cost maps.  An extension BESIDE the other headers: nothing in them changes, NASTAR_VERSION stays
 * what it is -- ask nastar_soft_fields_abi().
 *
 * Moves and costs are those of nastar_fields.h: a move n -> m = n + off is allowed when off is in the 9-bit neighbor_mask, m is inside the
 * map and m is passable; it costs cost[n], the cell being LEFT.  A goal on an obstacle is 0 in the output and is never entered.  Per map the
 * inputs are cost[H,W], goal[H,W] (EVERY non-zero cell is a goal), passable[H,W], a temperature tau > 0 and a horizon K >= 1.
 *
 *   softmin    softmin_tau(x) = x_min - tau * log(sum of exp(-(x_i - x_min) / tau)) over the finite x_i; +inf when none is finite.
 *   field      V_0(n) = 0 on passable goals and +inf elsewhere.  For k = 1..K, from V_{k-1} ONLY (Jacobi: two planes, no in-place update):
 *              V_k(n) = 0 on passable goals, +inf on obstacles, otherwise cost[n] + softmin_tau over the allowed moves n -> m of V_{k-1}(m).
 *              So V_k(n) = -tau * log(sum of exp(-cost(p) / tau)) over the routes p from n that first reach a goal within k moves.  Exactly K
 *              sweeps run: the field is defined for every cost >= 0, every tau > 0 and every K, and no trip count depends on the data.  The
 *              result is a pure function of the inputs: two calls give the same bits, whatever order the hardware ran the wavefronts in.
 *   output     dist = V_K: 0 on EVERY goal cell (a goal on an obstacle too), +inf on obstacles and where no goal lies within K moves.
 *   policy     [8,H,W] fp32, action k = the planning-datasets order (-1,0) (0,1) (0,-1) (1,0) (-1,1) (-1,-1) (1,1) (1,-1) as (dy, dx):
 *              pi_K(a|n) = the softmax, over the allowed moves with a finite target, of -V_{K-1}(m) / tau.  All-zero on goals, obstacles and
 *              cells with V_K = +inf.
 *   status     per map, int32: NASTAR_OK; NASTAR_ERR_BAD_COST (9, nastar_fields.h) for a passable cell with a NaN or a negative cost (-0.0 is
 *              fine; obstacle cells are not looked at): that map gets all +inf and zero policies and is reported before a missing goal, the
 *              other maps of the batch are computed; NASTAR_ERR_UNSOLVABLE (3) for a map without a goal cell (all +inf).  Zero costs are
 *              fine: there is no plateau here.
 *   tape       what the backward reads: the planes V_1 .. V_K of every map, in units the library chooses (B * K * H * W fp32,
 *              nastar_soft_fields_tape_bytes).  Without a tape pointer nothing but dist, policy and status is written.
 *
 * The vector-Jacobian product, nastar_soft_fields_backward, with an upstream gradient grad_dist[H,W]:
 *
 *   live       a cell is live at step k when it is passable, not a goal, and V_k is finite there.
 *   A          A_K = grad_dist READ ON THE CELLS LIVE AT K ONLY: a NaN or an infinity elsewhere reaches no output (the rule of
 *              nastar_fields_grad.h).  For k = K..1: grad_cost(n) += A_k(n), and A_{k-1}(m) = the sum over the predecessors n of m of
 *              pi_k(m|n) * A_k(n) on the cells live at k - 1, 0 elsewhere -- a GATHER at m over the allowed moves n -> m, with pi_k(.|n) the
 *              softmax of -V_{k-1}(.) / tau over n's allowed finite targets.  (What steps onto a goal is absorbed there.)
 *   order      the predecessors of m are added one after the other in the order of their position relative to m: (-1,-1) (-1,0) (-1,1)
 *              (0,-1) (0,1) (1,-1) (1,0) (1,1) as (dy, dx) -- row-major.  No floating-point atomics: two calls give the same bits.
 *   rounding   the sum over k is accumulated in fp64 and rounded once, at the store (the rule of the replay backward).
 *   output     grad_cost[n] is exactly 0.0f on a cell that was never live.  For a one-hot grad_dist at a start cell it is the expected
 *              number of visits of the stochastic policy pi on its way to a goal.
 *   status     per map, int32: NASTAR_OK, or NASTAR_ERR_BAD_COST (an all-zero grad_cost).
 *
 * One workgroup owns one map and keeps its planes in LDS: maps of more than nastar_soft_fields_max_cells() cells are refused, and the backward
 * refuses maps of more than nastar_soft_fields_grad_max_cells().  No gradient flows through the policy or to tau.
 */
#ifndef NASTAR_SOFT_FIELDS_H_
#define NASTAR_SOFT_FIELDS_H_

#include "nastar_fields.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NASTAR_SOFT_FIELDS_ABI 1

/* 1: the definition above */
int nastar_soft_fields_abi(void);

/* the largest H*W nastar_soft_cost_to_go takes (12288: the cost and two planes of one map in the LDS of one workgroup) */
int nastar_soft_fields_max_cells(void);

/* the largest H*W nastar_soft_fields_backward takes (6144) */
int nastar_soft_fields_grad_max_cells(void);

/* the bytes of the tape of a call: B * horizon * H * W * 4; 0 when an argument is below 1, SIZE_MAX when the product does not fit */
size_t nastar_soft_fields_tape_bytes(int B, int H, int W, int horizon);

/* cost, goal, passable: [B,H,W] fp32, device; dist_out [B,H,W] fp32; policy_out [B,8,H,W] fp32 or NULL (no policy is written); status_out [B]
 * int32; tape: device memory of tape_bytes >= nastar_soft_fields_tape_bytes(B, H, W, horizon) bytes, 16-byte aligned, or NULL (tape_bytes is
 * not looked at).  One launch on `stream`.  Refused before any HIP call, in this order: an invalid neighbor_mask (NASTAR_ERR_UNSUPPORTED); a
 * NULL cost / goal / passable / dist_out / status_out (NASTAR_ERR_NULL); B, H, W or horizon < 1, or a tau that is not finite and positive
 * (NASTAR_ERR_BAD_SHAPE); H*W above nastar_soft_fields_max_cells() (NASTAR_ERR_UNSUPPORTED); a tape that is too small or misaligned
 * (NASTAR_ERR_WORKSPACE). */
int nastar_soft_cost_to_go(const float* cost, const float* goal, const float* passable, int B, int H, int W, unsigned neighbor_mask, double tau,
                           int horizon, float* dist_out, float* policy_out, int32_t* status_out, void* tape, size_t tape_bytes, void* stream);

/* cost, goal, passable, neighbor_mask, tau, horizon: those of the nastar_soft_cost_to_go call that wrote `tape`; grad_dist [B,H,W] fp32;
 * grad_cost_out [B,H,W] fp32; status_out [B] int32.  One launch on `stream`, nothing is read back.  Refused before any HIP call, in this
 * order: an invalid neighbor_mask (NASTAR_ERR_UNSUPPORTED); a NULL cost / goal / passable / tape / grad_dist / grad_cost_out / status_out
 * (NASTAR_ERR_NULL); B, H, W or horizon < 1, or a tau that is not finite and positive (NASTAR_ERR_BAD_SHAPE); H*W above
 * nastar_soft_fields_grad_max_cells() (NASTAR_ERR_UNSUPPORTED); a tape that is too small or misaligned (NASTAR_ERR_WORKSPACE). */
int nastar_soft_fields_backward(const float* cost, const float* goal, const float* passable, const void* tape, size_t tape_bytes,
                                const float* grad_dist, int B, int H, int W, unsigned neighbor_mask, double tau, int horizon,
                                float* grad_cost_out, int32_t* status_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NASTAR_SOFT_FIELDS_H_ */
