/* nastar_fields_grad.h -- the gradient of the cost-to-go field with respect to the cost maps: the vector-Jacobian product of
 * nastar_cost_to_go (include/nastar_fields.h).  An extension BESIDE the other headers: nothing in them changes, NASTAR_VERSION stays what it
 * is -- ask nastar_fields_grad_abi().
 *
 * Along the policy the field is D(n) = fl32(cost[n] + D(s(n))), so dD(n)/dcost[v] is 1 when v lies on the policy roll-out from n (n itself
 * included, the goal it ends in excluded) and 0 otherwise: the product with an upstream gradient is a SUBTREE SUM over the policy forest.
 * Per map the inputs are dist[H,W] as nastar_cost_to_go wrote it, goal[H,W], passable[H,W], the 9-bit neighbor_mask of that call and the
 * upstream gradient grad_dist[H,W].
 *
 *   readable   what a move into m reads: dist[m] where passable[m] is non-zero, +inf elsewhere -- an obstacle is never entered, a goal on an
 *              obstacle neither, as in the forward kernel.
 *   successor  s(n) is the move the policy of nastar_fields.h takes at n: the FIRST action, in the planning-datasets order (-1,0) (0,1)
 *              (0,-1) (1,0) (-1,1) (-1,-1) (1,1) (1,-1) as (dy, dx), among the allowed moves n -> m (inside the map, in the mask) whose
 *              target has the smallest readable value -- taken only if that value is strictly below dist[n].  It is recomputed from dist,
 *              goal and passable: the [8,H,W] policy planes are not an input.
 *   live       a cell with goal[n] == 0 and a finite dist[n].  (Goals, obstacles and unreachable cells are not live.)
 *   A          for a live v: A(v) = G(v) + sum of A(c) over the live cells c with s(c) = v, where G is grad_dist READ ON LIVE CELLS ONLY:
 *              grad_dist on goals, obstacles and unreachable cells never enters a sum, a NaN or an infinity there reaches no output.
 *   output     grad_cost[v] = fl32(A(v)) on live cells and exactly 0.0f everywhere else.
 *   rounding   A is accumulated in fp64 and rounded once, at the store (the rule of the replay backward).
 *   order      the children of v are added to G(v) one after the other in the order of their position relative to v: (-1,-1) (-1,0)
 *              (-1,1) (0,-1) (0,1) (1,-1) (1,0) (1,1) as (dy, dx) -- row-major.  With that the result is a pure function of the inputs:
 *              two calls give the same bits, whatever order the hardware ran the wavefronts in.  (No floating-point atomics.)
 *   status     per map, int32: NASTAR_OK; NASTAR_ERR_PLATEAU (11) when a live cell has NO successor -- a zero-cost plateau, or a cell whose
 *              fl32(cost + D) did not rise above D: the field does not depend on that cell's cost the way the formula above says.  That map
 *              gets an all-zero grad_cost, the other maps of the batch are computed.  A map without a goal (a field of +inf) has no live
 *              cell: all zeros, NASTAR_OK.  NASTAR_ERR_NO_CONVERGENCE (10, nastar_fields.h) when the sweep bound H*W was hit: impossible,
 *              since s strictly lowers dist and the forest is therefore at most H*W - 2 edges high; it exists so that the loop has a bound
 *              no input can move.
 *
 * One workgroup owns one map and keeps A in LDS: maps of more than nastar_fields_grad_max_cells() cells are refused.
 */
#ifndef NASTAR_FIELDS_GRAD_H_
#define NASTAR_FIELDS_GRAD_H_

#include "nastar_fields.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NASTAR_FIELDS_GRAD_ABI 1

/* per-map status code of this header only (nastar_fields.h ends at 10) */
#define NASTAR_ERR_PLATEAU 11  /* a live cell without a strictly closer neighbour */

/* 1: the definition above */
int nastar_fields_grad_abi(void);

/* the largest H*W nastar_fields_backward takes (16384: every size nastar_cost_to_go takes) */
int nastar_fields_grad_max_cells(void);

/* dist, goal, passable, grad_dist: [B,H,W] fp32, device; grad_cost_out [B,H,W] fp32; status_out [B] int32; sweeps_out [B] int32 or NULL: the
 * sweeps every map's accumulation took, the quiet one included (0 for a map that skipped the loop; the count depends on the order the
 * hardware ran the wavefronts in, the gradient does not).  One launch on `stream`, no workspace.  Refused before any HIP call, in this
 * order: an invalid neighbor_mask (NASTAR_ERR_UNSUPPORTED), a NULL dist / goal / passable / grad_dist / grad_cost_out / status_out
 * (NASTAR_ERR_NULL), B, H or W < 1 (NASTAR_ERR_BAD_SHAPE), H*W above nastar_fields_grad_max_cells() (NASTAR_ERR_UNSUPPORTED). */
int nastar_fields_backward(const float* dist, const float* goal, const float* passable, const float* grad_dist, int B, int H, int W,
                           unsigned neighbor_mask, float* grad_cost_out, int32_t* status_out, int32_t* sweeps_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NASTAR_FIELDS_GRAD_H_ */
