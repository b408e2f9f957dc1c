/* nastar_sources.h -- the search from SEVERAL start cells per map (multi-source A*): a third header BESIDE include/nastar.h and
 * include/nastar_routes.h (libnastar_hip.so exports all three; nothing in the other two changes and NASTAR_VERSION stays what it is -- ask
 * nastar_sources_abi()).
 *
 * Every search entry point of nastar.h and nastar_routes.h reads `start` as a one-hot map: of several non-zero cells it takes the one with
 * the highest flat index and says nothing.  The reference's forward() never asks for a one-hot start map -- its open list simply begins as
 * open_maps = start_maps -- so a map with K start cells is searched from all of them at once ("the nearest of K depots").  The entry points
 * below do that.  Per map, with S = the non-zero cells of start[b] (values are expected in {0, 1}; any non-zero value counts):
 *
 *   initial state   every s in S is open with g = 0 and an unset parent, on an obstacle too; its key comes from
 *                   f = fl(fl(g_ratio 0) + fl((1 - g_ratio) fl(h0(s) + cost(s)))) like any open cell's.  Two starts with equal keys are a tie
 *                   like any other: the lower flat index is selected first.
 *   steps           unchanged: an unselected start is an ordinary open cell (with a negative cost next to it, it can be re-parented).
 *   parent walks    (paths_out, the routes, the lock-step FINAL launch) end at the first cell whose parent is unset, or at their hop cap --
 *                   not "at the start": the route begins at the source that reached the goal and may pass through another start cell.
 *   status          no non-zero start cell or no goal: NASTAR_ERR_UNSOLVABLE for that map, as in nastar.h; so is a map whose open list runs
 *                   empty before the goal is selected (all of its starts walled in).  The other maps of the batch are searched.
 *   replay          the initial softmax sums run over S: every start is open from history index 0.
 *
 * A one-hot start map gives bit-identical outputs to nastar_forward_routes / nastar_forward_ex_heuristic / nastar_forward_ex_masked with the same
 * mask.  The kernels are the compiled step loops and the large-map kernel with a seeding pass in front (csrc/nastar_forward_compact_body.inc,
 * csrc/nastar_forward_hybrid_body.inc); the hand-scheduled streams and the unit-cost layout take no start set (NASTAR_FLAG_UNIT_COST is accepted
 * and has no effect).  The workspace sizes are those of nastar.h: nastar_workspace_bytes / nastar_batchloop_workspace_bytes /
 * nastar_backward_workspace_bytes.
 */
#ifndef NASTAR_SOURCES_H_
#define NASTAR_SOURCES_H_

#include "nastar.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NASTAR_SOURCES_ABI 1

/* 1: the semantics described above */
int nastar_sources_abi(void);

/* The argument list of nastar_forward_routes.  h0 may be NULL (the reference's heuristic).  The route outputs may all be NULL: no routes are
 * written (routes_out NULL decides; the other three are then ignored).  routes_out given without route_len_out: NASTAR_ERR_NULL; with
 * route_cap < 1: NASTAR_ERR_BAD_SHAPE; an invalid neighbor_mask: NASTAR_ERR_UNSUPPORTED -- all refused before any HIP call.  Everything else
 * as nastar_forward_ex. */
int nastar_forward_sources(const float* cost, const float* start, const float* goal, const float* passable, int B, int H, int W, double g_ratio,
                           int max_iters, float* histories_out, int64_t* paths_out, int32_t* sel_log_out, int32_t* iters_out, int32_t* status_out,
                           uint8_t* packed_out, void* workspace, size_t workspace_bytes, int flags, const int32_t* order, int32_t* order_out,
                           int32_t* status_summary, int32_t* completion_counter, unsigned neighbor_mask, const float* h0, int32_t* routes_out,
                           int route_cap, int32_t* route_len_out, float* route_cost_out, void* stream);

/* The argument list of nastar_forward_routes_batchloop_finish, behind a nastar_forward_sources launch with NASTAR_FLAG_MARK_COUPLED (same
 * arguments, same workspace): the PROBE and FINAL launches open every start cell too.  The same refusals. */
int nastar_forward_sources_batchloop_finish(const float* cost, const float* start, const float* goal, const float* passable, int B, int H, int W,
                                            double g_ratio, int max_iters, float* histories_out, int64_t* paths_out, int32_t* sel_log_out,
                                            int32_t* iters_out, int32_t* status_out, void* workspace, size_t workspace_bytes,
                                            unsigned neighbor_mask, const float* h0, int32_t* routes_out, int route_cap, int32_t* route_len_out,
                                            float* route_cost_out, void* stream);

/* The argument list of nastar_backward_replay_ordered_heuristic; h0 may be NULL.  Replays the selection log of a nastar_forward_sources search
 * (NASTAR_FLAG_LOCKSTEP for a log the batch-loop finish completed).  The compiled replay loops (LDS state or HBM state) only. */
int nastar_backward_replay_sources(const float* grad_histories, const float* histories, const float* opt_trajs, const float* grad_loss_dev,
                                   const float* cost, const float* start, const float* goal, const float* passable, const int32_t* sel_log,
                                   int B, int H, int W, double g_ratio, int max_iters, const int32_t* iters, const int32_t* t_batch_dev,
                                   float* grad_cost_out, void* workspace, size_t workspace_bytes, int flags, const int32_t* order,
                                   unsigned neighbor_mask, const float* h0, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NASTAR_SOURCES_H_ */
