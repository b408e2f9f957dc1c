/* nastar_fields.h -- the exact cost-to-go FIELD of whole maps and the optimal policy that follows it: an extension BESIDE include/nastar.h
 * (libnastar_hip.so exports both; nothing in nastar.h changes and NASTAR_VERSION stays what it is -- ask nastar_fields_abi()).
 *
 * The search entry points answer a question about one start and one goal.  This one answers "what does it cost to reach the goal from
 * EVERYWHERE" under the search's own cost semantics.  Per map: cost[H,W] fp32, passable[H,W] (non-zero = enterable), goal[H,W] (EVERY
 * non-zero cell is a goal: K >= 1 goals give the nearest of K) and a 9-bit neighbor_mask (NASTAR_NEIGHBORS_* of nastar.h).
 *
 *   moves    n -> m = n + off, off one of the offsets the search opens from a selected cell under that mask (bit a*3+b <=> offset
 *            (1-a, 1-b)); m inside the map and passable.  The move costs cost[n]: the cell being LEFT, what the search's g adds up.
 *   field    D(goal cell) = 0, passable or not.  D(n) = +inf for a non-goal obstacle cell and for a cell no goal can be reached from.
 *            Otherwise D(n) = min over the allowed moves n -> m of fl32(cost[n] + D(m)): the fixed point that relaxing from "+inf
 *            everywhere but the goals" ends in.  x -> fl32(c + x) is monotone and costs are >= 0, so it is the same BITS in whatever order
 *            the cells are relaxed.  (A goal on an obstacle cell cannot be entered: only that cell is 0.)
 *   policy   [8,H,W] one-hot fp32, action k = the planning-datasets "moore" order (-1,0) (0,1) (0,-1) (1,0) (-1,1) (-1,-1) (1,1) (1,-1)
 *            as (dy, dx).  A cell with finite D(n) > 0 takes the first k, in that order, among the allowed moves whose target has the
 *            smallest D(m) -- if that D(m) is below D(n).  All-zero on goals, obstacles, unreachable cells, and on a cell whose best
 *            neighbour is not strictly closer (possible with zero costs only: a plateau has no downhill move).
 *   status   per map, int32: NASTAR_OK; NASTAR_ERR_UNSOLVABLE (3) for a map without a goal cell (field all +inf, policy all zero);
 *            NASTAR_ERR_BAD_COST for a passable cell with a NaN or a negative cost (-0.0 is fine; obstacle cells are not looked at): that map
 *            gets all +inf and zero policies and is reported before a missing goal, the other maps of the batch are computed;
 *            NASTAR_ERR_NO_CONVERGENCE when the sweep bound H*W was hit -- impossible for accepted inputs, it exists so that the loop has a
 *            bound no input can move.
 *
 * g_ratio, Tmax and the heuristic play no part.  One workgroup relaxes one map in LDS: maps of more than nastar_fields_max_cells() cells are
 * refused.
 */
#ifndef NASTAR_FIELDS_H_
#define NASTAR_FIELDS_H_

#include "nastar.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NASTAR_FIELDS_ABI 1

/* per-map status codes of this header only (nastar.h ends at 8) */
#define NASTAR_ERR_BAD_COST 9         /* a NaN or a negative cost on a passable cell */
#define NASTAR_ERR_NO_CONVERGENCE 10  /* H*W sweeps without a quiet one */

/* 1: the definition above */
int nastar_fields_abi(void);

/* the largest H*W nastar_cost_to_go takes (16384: field + cost of one map in the LDS of one workgroup) */
int nastar_fields_max_cells(void);

/* cost, goal, passable: [B,H,W] fp32, device; dist_out [B,H,W] fp32; policy_out [B,8,H,W] fp32 or NULL (no policy is computed); status_out
 * [B] int32.  One launch on `stream`, no workspace.  Refused before any HIP call: an invalid neighbor_mask (NASTAR_ERR_UNSUPPORTED), a NULL
 * cost / goal / passable / dist_out / status_out (NASTAR_ERR_NULL), B, H or W < 1 (NASTAR_ERR_BAD_SHAPE), H*W above
 * nastar_fields_max_cells() (NASTAR_ERR_UNSUPPORTED). */
int nastar_cost_to_go(const float* cost, const float* goal, const float* passable, int B, int H, int W, unsigned neighbor_mask, float* dist_out,
                      float* policy_out, int32_t* status_out, void* stream);

/* nastar_cost_to_go that also writes, per map, the number of sweeps its relaxation took, the quiet one included (sweeps_out [B] int32, may be
 * NULL; 0 for a map that skipped the loop).  For probes: the count depends on the order the hardware ran the wavefronts in, the field does
 * not. */
int nastar_cost_to_go_sweeps(const float* cost, const float* goal, const float* passable, int B, int H, int W, unsigned neighbor_mask,
                             float* dist_out, float* policy_out, int32_t* status_out, int32_t* sweeps_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NASTAR_FIELDS_H_ */
