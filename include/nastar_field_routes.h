/* nastar_field_routes.h -- ordered optimal routes for MANY start cells per map, read off a cost-to-go field.  A tenth header BESIDE the
 * others: nothing in them changes, NASTAR_VERSION stays what it is -- ask nastar_field_routes_abi().
 *
 * A field (include/nastar_fields.h, nastar_fields_tiled.h) answers "what does it cost from everywhere".  This header answers what follows
 * from it: which cells does one drive through from here -- for S start cells per map, from ONE field per map, without a search.  As the
 * opening of nastar_routes.h says, a 0/1 mask gives no order with 8-connected moves: the answer is a list of cells.
 *
 * Per map the inputs are dist[H,W] as nastar_cost_to_go or nastar_cost_to_go_tiled wrote it, goal[H,W], passable[H,W], the 9-bit
 * neighbor_mask of that call, and start_idx[S]: int32 flat cell indices r*W + c.
 *
 *   readable, successor   those of include/nastar_fields_grad.h, word for word: a move into m reads dist[m] where passable[m] is non-zero and
 *              +inf elsewhere; s(n) is the FIRST action, in the planning-datasets order, among the allowed in-map moves whose target has the
 *              smallest readable value -- taken only if that value is strictly below dist[n].  A cell whose dist is not finite has none.
 *   route      for query (b, s) with start cell n0: n0, s(n0), s(s(n0)), ... up to and including the first cell with goal != 0.  A start
 *              on a goal cell gives [n0], passable or not (the field holds 0 there).  s strictly lowers dist, so a route has at most H*W
 *              cells: the loop carries that bound, which no input can move.
 *   route_len_out[b,s]    int32: the TRUE number of route cells, also when the row is too short.
 *   routes_out[b,s,:]     int32 [route_cap], the convention of nastar_routes.h: entries [0, min(len, cap)) hold the LAST min(len, cap) cells
 *              of the route in travel order, the goal last; every entry behind them is -1 (the row is fully written).  May be NULL: the
 *              call then returns lengths, costs and status only.
 *   route_cost_out[b,s]   float32 (may be NULL): dist[n0], the field's own bits -- +inf for an obstacle or an unreachable start, and +inf
 *              when start_idx is out of range.
 *   status_out[b,s]       int32, looked at in this order:
 *                NASTAR_ERR_BAD_SHAPE (1)    start_idx outside [0, H*W)
 *                NASTAR_ERR_UNSOLVABLE (3)   dist[n0] is not finite (an obstacle, an unreachable cell, a NaN)
 *                NASTAR_ERR_PLATEAU (11)     the chain reaches a cell that is no goal and has no successor (a zero-cost plateau)
 *                NASTAR_OK (0)
 *              Every failed query has len 0 and a row of -1; the other queries of the map and the other maps are unaffected.
 *
 * How: one byte per cell holds the successor's action 0..7, a mark for a goal cell, or "none".  Up to nastar_field_routes_lds_cells() cells
 * the call is ONE launch: a workgroup builds its map's whole table in LDS and each of its lanes chases one start through it; the starts of
 * a map are split over several workgroups, which rebuild the table independently -- no workgroup waits for another.  Above that limit the
 * table is written to the workspace by a first launch and chased from there by a second.  The -1 of the rows are one memset of routes_out
 * in front of the launches.  Nothing is read back: the call does not block and can be captured into a graph.
 */
#ifndef NASTAR_FIELD_ROUTES_H_
#define NASTAR_FIELD_ROUTES_H_

#include "nastar_fields_grad.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NASTAR_FIELD_ROUTES_ABI 1

/* 1: the definition above */
int nastar_field_routes_abi(void);

/* the largest H*W nastar_field_routes takes: 1179648, the limit of nastar_cost_to_go_tiled -- every map a field exists for can be routed */
int nastar_field_routes_max_cells(void);

/* the largest H*W whose successor table is kept in LDS (one launch, no workspace): 163840 */
int nastar_field_routes_lds_cells(void);

/* bytes of workspace (device memory) a call on B maps of H x W needs: 0 up to nastar_field_routes_lds_cells() cells -- `workspace` may then
 * be NULL -- and B*H*W rounded up to 16 above; also 0 for B, H or W < 1 and for H*W above nastar_field_routes_max_cells() */
size_t nastar_field_routes_workspace_bytes(int B, int H, int W);

/* dist, goal, passable: [B,H,W] fp32, device; start_idx [B,S] int32; routes_out [B,S,route_cap] int32 or NULL; route_len_out [B,S] int32;
 * route_cost_out [B,S] fp32 or NULL; status_out [B,S] int32.  Enqueued on `stream`, no host read.  Refused before any HIP call, in this
 * order: an invalid neighbor_mask (NASTAR_ERR_UNSUPPORTED), a NULL dist / goal / passable / start_idx / route_len_out / status_out
 * (NASTAR_ERR_NULL), B, S, H or W < 1, or route_cap < 1 with a non-NULL routes_out (NASTAR_ERR_BAD_SHAPE), H*W above
 * nastar_field_routes_max_cells() or B*S above 2^30 (NASTAR_ERR_UNSUPPORTED), workspace_bytes below nastar_field_routes_workspace_bytes or a
 * NULL workspace where that is not 0 (NASTAR_ERR_WORKSPACE).  After a HIP error nothing more is launched and NASTAR_ERR_HIP is returned. */
int nastar_field_routes(const float* dist, const float* goal, const float* passable, const int32_t* start_idx, int B, int S, int H, int W,
                        unsigned neighbor_mask, int32_t* routes_out, int route_cap, int32_t* route_len_out, float* route_cost_out,
                        int32_t* status_out, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NASTAR_FIELD_ROUTES_H_ */
