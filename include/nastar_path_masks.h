/* nastar_path_masks.h -- the exact shortest path of every map as a 0/1 MASK, and its blackbox gradient with respect to the cost map, one
 * launch each.  An eleventh header BESIDE the others: nothing in them changes, NASTAR_VERSION stays what it is -- ask nastar_path_masks_abi().
 *
 * nastar_cost_to_go answers "what does it cost from everywhere", nastar_field_routes "which cells from these starts".  A training loop that
 * uses the exact solver as a LAYER (blackbox differentiation, Vlastelica et al. 2020: the "BB-A*" baseline of the Neural A* paper) needs less
 * and needs it twice per step: ONE start per map, the route as a mask, no field or policy planes in memory.  Per map the inputs are
 * cost[H,W], goal[H,W], passable[H,W] fp32 and the 9-bit neighbor_mask as nastar_cost_to_go takes them, and start_idx: ONE int32 flat cell
 * index r*W + c.
 *
 *   field      D of include/nastar_fields.h, word for word and bit for bit: the same relaxation to the same fixed point.
 *   route      that of include/nastar_field_routes.h, word for word: n0, s(n0), s(s(n0)), ... up to and including the first goal cell, s(n)
 *              the FIRST action, in the planning-datasets order, among the allowed in-map moves whose target has the smallest readable
 *              value, taken only if that value is strictly below D(n).  s strictly lowers D: the loop carries the bound H*W.
 *   path_out[b,:,:]    fp32: 1 on the start, on the goal cell reached and on every cell between them, 0 elsewhere (the convention of the
 *              search's paths_out).  Every cell is written.
 *   path_cost_out[b]   fp32 (may be NULL): D(n0), the field's own bits; +inf for a failed map.
 *   status_out[b]      int32, looked at in this order:
 *                NASTAR_ERR_BAD_SHAPE (1)        start_idx outside [0, H*W)
 *                NASTAR_ERR_BAD_COST (9)         a NaN or a negative cost on a passable cell
 *                NASTAR_ERR_UNSOLVABLE (3)       no goal cell, or D(n0) is not finite (an obstacle, an unreachable start)
 *                NASTAR_ERR_NO_CONVERGENCE (10)  the sweep bound H*W was hit (impossible for accepted inputs)
 *                NASTAR_ERR_PLATEAU (11)         the chain reaches a cell that is no goal and has no successor (a zero-cost plateau)
 *                NASTAR_OK (0)
 *              A failed map has an all-zero mask and a cost of +inf; the other maps of the batch are unaffected.
 *
 * The BLACKBOX GRADIENT of a loss L(path) with respect to the costs is (y(w') - y(w)) / lambda with w' = w + lambda * dL/dy: a second exact
 * solve.  nastar_path_masks_backward perturbs on load, in two separately rounded fp32 operations and a clamp:
 *       w'[n] = fmaxf(fl32(fl32(lambda * grad_path[n]) + cost[n]), min_cost)        (a NaN stays a NaN: the map then fails with BAD_COST)
 * solves and chases as above, and stores
 *       grad_cost_out[n] = (y'[n] - path_fwd[n]) * inv_lambda,   inv_lambda = fl32(1 / lambda)
 * -- exactly 0 or +-inv_lambda for a 0/1 path_fwd.  A map whose status_fwd is not NASTAR_OK gets an all-zero row (nothing is solved); a map
 * whose PERTURBED solve fails gets an all-NaN row: loud, and without a host read.
 *
 * How: one workgroup owns one map, as in nastar_cost_to_go; field and cost live in LDS; after the relaxation one lane chases the route and
 * marks its cells in the LDS cost array, which is free by then; behind one barrier all lanes store the map's row, coalesced -- every cell
 * of the output is written by that pass alone.  Maps of more than nastar_path_masks_max_cells() cells are refused: the tiled composition
 * (nastar_cost_to_go_tiled, nastar_field_routes, a scatter) is not built into this call.  Nothing is read back: both calls are enqueued,
 * do not block and can be captured into a graph.
 */
#ifndef NASTAR_PATH_MASKS_H_
#define NASTAR_PATH_MASKS_H_

#include "nastar_field_routes.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NASTAR_PATH_MASKS_ABI 1

/* 1: the definition above */
int nastar_path_masks_abi(void);

/* the largest H*W both calls take: 16384, the one-workgroup limit of nastar_cost_to_go */
int nastar_path_masks_max_cells(void);

/* cost, goal, passable: [B,H,W] fp32, device; start_idx [B] int32; path_out [B,H,W] fp32; path_cost_out [B] fp32 or NULL; status_out [B]
 * int32.  One launch on `stream`, no workspace, no host read.  Refused before any HIP call, in this order: an invalid neighbor_mask
 * (NASTAR_ERR_UNSUPPORTED), a NULL cost / goal / passable / start_idx / path_out / status_out (NASTAR_ERR_NULL), B, H or W < 1
 * (NASTAR_ERR_BAD_SHAPE), H*W above nastar_path_masks_max_cells() (NASTAR_ERR_UNSUPPORTED). */
int nastar_path_masks(const float* cost, const float* goal, const float* passable, const int32_t* start_idx, int B, int H, int W,
                      unsigned neighbor_mask, float* path_out, float* path_cost_out, int32_t* status_out, void* stream);

/* the inputs of nastar_path_masks; grad_path [B,H,W] fp32: the upstream gradient of path_out; path_fwd [B,H,W] fp32 and status_fwd [B]
 * int32: path_out and status_out as nastar_path_masks wrote them; lambda > 0: the interpolation step; min_cost > 0: the clamp of the
 * perturbed costs; grad_cost_out [B,H,W] fp32; status_out [B] int32 or NULL: the status of the PERTURBED solve, NASTAR_OK for a map that
 * status_fwd skipped.  One launch on `stream`, no workspace, no host read.  Refused before any HIP call, in this order: an invalid
 * neighbor_mask (NASTAR_ERR_UNSUPPORTED), a NULL cost / goal / passable / start_idx / grad_path / path_fwd / status_fwd / grad_cost_out
 * (NASTAR_ERR_NULL), B, H or W < 1 (NASTAR_ERR_BAD_SHAPE), H*W above nastar_path_masks_max_cells(), or a lambda or min_cost that is not a
 * finite positive number, or a lambda whose fp32 reciprocal is not finite (NASTAR_ERR_UNSUPPORTED). */
int nastar_path_masks_backward(const float* cost, const float* goal, const float* passable, const int32_t* start_idx,
                               const float* grad_path, const float* path_fwd, const int32_t* status_fwd, int B, int H, int W,
                               unsigned neighbor_mask, float lambda, float min_cost, float* grad_cost_out, int32_t* status_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NASTAR_PATH_MASKS_H_ */
