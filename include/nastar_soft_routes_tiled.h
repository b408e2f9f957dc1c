/* nastar_soft_routes_tiled.h -- SAMPLED routes from the maximum-entropy route distribution (include/nastar_soft_routes.h) for maps of up to
 * nastar_soft_routes_tiled_max_cells() cells, read from the CHECKPOINTED tape of include/nastar_soft_fields_tiled.h.  A nineteenth header
 * BESIDE the others: nothing in them changes, NASTAR_VERSION stays what it is -- ask nastar_soft_routes_tiled_abi().
 *
 * Definition: nothing new.  The walker, its candidates, the fp32 weights exp2(U_min - U) in action order, t = fl32(u * Z), "the first
 * running sum > t, else the last candidate", the Philox counter (j, i, q, 0) and its key, uniforms[b,s,i,j]; the fp64 sums of route_cost and
 * log_prob rounded once, visits by integer atomics, the rows (the last min(len, cap) cells, the goal last, -1 behind), the statuses 1 / 9 / 3
 * in that order, a start on a goal and a failed query's outputs: as in nastar_soft_routes.h, word for word.  The move of a walker is the
 * one-workgroup kernels' own statements, and the planes are the forward's bits, so on every map both entry points take every output is the
 * same BITS as nastar_soft_routes writes, whatever checkpoint_every is.
 *
 * What differs is where the planes come from.  The tape holds the planes at the multiples of checkpoint_every = c and plane K.  The walker
 * with k moves left reads plane k - 1: the call goes through the tape's segments from the top, as nastar_soft_fields_backward_tiled does.
 *
 *   prepare    one launch writes the per-map flags (which stand in for the one-workgroup kernel's scan of the map), the costs in units
 *              and V_0; one launch writes the -1 of the rows and the zeros of visits_out.
 *   segment    for every segment lo < k <= hi, top down: the forward's sweeps rebuild the planes lo + 1 .. hi - 1 from the checkpoint lo
 *              (segment 0 from V_0) into a buffer of at most c - 1 planes, then ONE launch of walkers, 256 to a workgroup, one per lane,
 *              advances every walker that is still on its way through the moves of the segment, gathering its eight values from device
 *              memory.  No workgroup waits for another; a wavefront whose walkers have all ended returns at once.
 *   state      between two launches a walker lives in the workspace: its cell, its length so far, whether it is on its way, its query's
 *              status and the two fp64 sums (32 bytes) -- the sums are the same sequence of additions as in one launch.  The draw is a
 *              pure function of (seed, q, i, j): a walk cut at any move and resumed in another launch is the same walk.  The first
 *              launch forms the status from V_K(n_0) in the tape's last slot and the flags; the last writes route_len_out,
 *              route_cost_out, log_prob_out and status_out.
 *   short rows a walk that may outgrow its row (route_cap < horizon + 1) is REPLAYED, first for the lengths, then for the stores, as the
 *              one-workgroup kernel replays it: here that means every segment is rebuilt TWICE.  Rows of horizon + 1 cells never pay it.
 *   cost       about one more forward (the rebuilt sweeps) and ceil(horizon / c) walker launches.
 *
 * The call only ENQUEUES on `stream`: nothing is read back, it does not block, and it uses no floating-point atomics.
 */
#ifndef NASTAR_SOFT_ROUTES_TILED_H_
#define NASTAR_SOFT_ROUTES_TILED_H_

#include "nastar_soft_fields_tiled.h"
#include "nastar_soft_routes.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NASTAR_SOFT_ROUTES_TILED_ABI 1

/* 1: the definition of nastar_soft_routes.h, computed as described above */
int nastar_soft_routes_tiled_abi(void);

/* the largest H*W nastar_soft_routes_tiled takes: nastar_soft_fields_tiled_max_cells() (1179648) */
int nastar_soft_routes_tiled_max_cells(void);

/* bytes of workspace (device memory, 16-byte aligned) a call needs: the per-map flags, the costs in units, V_0,
 * min(checkpoint_every, horizon) - 1 planes of the segment buffer and 32 bytes per walker; 0 when an argument is below 1, SIZE_MAX when it
 * does not fit */
size_t nastar_soft_routes_tiled_workspace_bytes(int B, int S, int N, int H, int W, int horizon, int checkpoint_every);

/* The arguments of nastar_soft_routes, with: tape / tape_bytes / checkpoint_every, what nastar_soft_cost_to_go_tiled wrote for these maps,
 * neighbor_mask, tau, horizon and checkpoint_every (tape_bytes >= nastar_soft_fields_tiled_tape_bytes(B, H, W, horizon, checkpoint_every),
 * 16-byte aligned); workspace / workspace_bytes >= nastar_soft_routes_tiled_workspace_bytes(B, S, N, H, W, horizon, checkpoint_every).
 * Refused before any HIP call, in this order: an invalid neighbor_mask (NASTAR_ERR_UNSUPPORTED); a NULL cost / goal / passable / tape /
 * start_idx / route_len_out / status_out / workspace (NASTAR_ERR_NULL); B, S, N, H, W, horizon or checkpoint_every < 1, a tau that is not
 * finite and positive, or route_cap < 1 with a non-NULL routes_out (NASTAR_ERR_BAD_SHAPE); H*W above
 * nastar_soft_routes_tiled_max_cells(), more than 2^24 tiles in the batch or B*S*N above 2^30 (NASTAR_ERR_UNSUPPORTED); a tape or a
 * workspace that is too small or misaligned (NASTAR_ERR_WORKSPACE).  After a failed launch nothing more is enqueued and NASTAR_ERR_HIP is
 * returned. */
int nastar_soft_routes_tiled(const float* cost, const float* goal, const float* passable, const void* tape, size_t tape_bytes,
                             int checkpoint_every, const int32_t* start_idx, int B, int S, int N, int H, int W, unsigned neighbor_mask,
                             double tau, int horizon, long long seed, const float* uniforms, int32_t* routes_out, int route_cap,
                             int32_t* route_len_out, float* route_cost_out, float* log_prob_out, int32_t* visits_out, int32_t* status_out,
                             void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NASTAR_SOFT_ROUTES_TILED_H_ */
