/* nastar_routes.h -- ordered routes, their lengths and costs from the search launch: an extension BESIDE include/nastar.h (libnastar_hip.so
 * exports both; nothing in nastar.h changes and NASTAR_VERSION stays what it is -- ask nastar_routes_abi()).
 *
 * The search entry points of nastar.h answer "which cells are on the path" as a 0/1 mask (paths_out).  With 8-connected moves a mask does
 * not determine an order.  The two entry points below run the SAME launches as nastar_forward_ex_heuristic /
 * nastar_forward_batchloop_finish_heuristic -- same kernels, same histories / paths / iters / status -- and also write, per map b:
 *
 *   route              the parent chain the backtrack marks, in travel order, the goal LAST; its cells are exactly the 1-cells of paths_out[b].
 *                        solved map                      start ... goal
 *                        budget ran out                  the chain the reference's backtrack marks with its cap (iters - 1 hops); need not begin at the start
 *                        goal never opened, start==goal  [goal]
 *                        no one-hot goal, or per-map status NASTAR_ERR_NOT_UNIT_COST / NASTAR_ERR_BAD_HEURISTIC     empty
 *   route_len_out[b]   int32: number of route cells (== sum of paths_out[b]) -- always the TRUE length, also when the row is too short
 *   routes_out[b, :]   int32 [route_cap]: entries [0, min(len, cap)) hold flat cell indices r*W + c -- the LAST min(len, cap) cells of the
 *                      route, so entry min(len, cap) - 1 is the goal; every entry behind them is -1 (the row is fully written).
 *                      route_cap = min(H*W, max_iters + 1) always suffices.
 *   route_cost_out[b]  float32 (optional, may be NULL): the sum, accumulated in double and rounded once, of cost[] over the route cells except
 *                      the goal -- the costs of the cells being LEFT, what the search's g accumulates.  Covers the whole route also when len > cap.
 *
 * Routes are indexed by MAP, never by workgroup: `order` / `order_out` work as in nastar_forward_ex.
 */
#ifndef NASTAR_ROUTES_H_
#define NASTAR_ROUTES_H_

#include "nastar.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NASTAR_ROUTES_ABI 1

/* 1: the layout described above */
int nastar_routes_abi(void);

/* nastar_forward_ex_heuristic + the route outputs.  h0 may be NULL (the reference's heuristic); with neighbor_mask == NASTAR_NEIGHBORS_MOORE8
 * and h0 == NULL the launch is exactly nastar_forward_ex's (hand-scheduled streams, unit-cost layout under NASTAR_FLAG_UNIT_COST), any other
 * mask nastar_forward_ex_masked's.  routes_out or route_len_out NULL: NASTAR_ERR_NULL; route_cap < 1: NASTAR_ERR_BAD_SHAPE; an invalid
 * neighbor_mask: NASTAR_ERR_UNSUPPORTED -- all refused before any HIP call.  Everything else as nastar_forward_ex. */
int nastar_forward_routes(const float* cost, const float* start, const float* goal, const float* passable, int B, int H, int W, double g_ratio,
                          int max_iters, float* histories_out, int64_t* paths_out, int32_t* sel_log_out, int32_t* iters_out, int32_t* status_out,
                          uint8_t* packed_out, void* workspace, size_t workspace_bytes, int flags, const int32_t* order, int32_t* order_out,
                          int32_t* status_summary, int32_t* completion_counter, unsigned neighbor_mask, const float* h0, int32_t* routes_out,
                          int route_cap, int32_t* route_len_out, float* route_cost_out, void* stream);

/* nastar_forward_batchloop_finish_heuristic + the route outputs, behind a nastar_forward_routes launch with NASTAR_FLAG_MARK_COUPLED (same
 * arguments, same workspace): the maps it re-runs in lock-step get their routes, lengths and costs rewritten with their other rows.
 * h0 may be NULL; the same refusals. */
int nastar_forward_routes_batchloop_finish(const float* cost, const float* start, const float* goal, const float* passable, int B, int H, int W,
                                           double g_ratio, int max_iters, float* histories_out, int64_t* paths_out, int32_t* sel_log_out,
                                           int32_t* iters_out, int32_t* status_out, void* workspace, size_t workspace_bytes,
                                           unsigned neighbor_mask, const float* h0, int32_t* routes_out, int route_cap, int32_t* route_len_out,
                                           float* route_cost_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NASTAR_ROUTES_H_ */
