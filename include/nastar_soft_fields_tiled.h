/* nastar_soft_fields_tiled.h -- the entropy-regularised cost-to-go field, its soft policy and its vector-Jacobian product
 * (include/nastar_soft_fields.h) for maps of up to nastar_soft_fields_tiled_max_cells() cells: TILED sweeps, and a tape with CHECKPOINTS.  A
 * fourteenth header BESIDE the others: nothing in them changes, NASTAR_VERSION stays what it is -- ask nastar_soft_fields_tiled_abi().
 *
 * Definition: nothing new.  The moves, the costs, the mask and the goal-on-an-obstacle rule; V_0, the K Jacobi sweeps, dist, policy, status
 * and its precedence; the adjoint with its live rule and its row-major gather order; the fp64 sum over k with one rounding at the store and
 * exactly 0.0f where a cell was never live: as there, word for word.  The cell update is the one-workgroup kernels' own (the same soft-min,
 * the same expressions in units of tau * ln 2), so dist, policy, status and grad_cost are the same BITS on every map both take (DESIGN.md
 * section 2, item 6m).  A cell outside the map reads as +inf, as the border tests of the one-workgroup sweep make it read.
 *
 * What differs is where the planes live and how a sweep reaches them:
 *
 *   planes     in device memory, in units; the map is cut into tiles (nastar_soft_fields_tile).  One PREPARE launch writes the per-map
 *              status, the bad-cost and no-goal flags, the costs in units and V_0.  Then ceil(K / S) launches cover every tile of every map:
 *              a workgroup loads its tile and a halo of S cells, runs S sweeps in LDS and stores the interior of the plane it reached (the
 *              last launch runs K mod S sweeps when that is not 0, and writes dist and the policy from the planes K - 1 and K it holds).
 *              Nothing is handed from one workgroup to another inside a launch: no workgroup waits for another, a value crosses a tile
 *              border at a kernel boundary.  The result does not depend on S.
 *   no read    both entry points only ENQUEUE on `stream`: nothing is read back and they do not block.
 *   tape       with a tape pointer the forward keeps the planes at the multiples of checkpoint_every = c >= 1 and plane K
 *              (horizon / c + 1 planes per map, nastar_soft_fields_tiled_tape_bytes; with c = 1, every plane).  The layout is the library's.
 *   backward   takes the same c.  Segment by segment, top down, it re-runs the forward sweeps from the segment's checkpoint (segment 0 from
 *              V_0, which comes from the inputs) into a segment buffer of at most c - 1 planes, then walks the segment back: ONE launch per
 *              step k, in which a workgroup rebuilds P = A_k / S_k and M_k on its tile and one halo cell from plane k - 1, gathers
 *              A_{k-1} on its interior in the stated order and adds it to the cell's fp64 sum in the workspace -- one workgroup owns a cell:
 *              no atomics.  A last launch rounds once into grad_cost.  The forward is a pure function, so the rebuilt planes are the
 *              forward's bits: grad_cost does not depend on c.
 */
#ifndef NASTAR_SOFT_FIELDS_TILED_H_
#define NASTAR_SOFT_FIELDS_TILED_H_

#include "nastar_soft_fields.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NASTAR_SOFT_FIELDS_TILED_ABI 1

/* 1: the definition of nastar_soft_fields.h, computed as described above */
int nastar_soft_fields_tiled_abi(void);

/* the largest H*W both entry points take: 1179648 (1024 x 1152, the limit of the search entry points) */
int nastar_soft_fields_tiled_max_cells(void);

/* the interior of a tile (*th x *tw cells) and S, the sweeps a launch runs (the halo of a tile is S cells); a NULL is not written; -> 0 */
int nastar_soft_fields_tile(int* th, int* tw, int* sweeps);

/* bytes of workspace (device memory, 16-byte aligned) a forward call on B maps of H x W needs: the costs in units, two planes and the
 * per-map flags; 0 when an argument is below 1, SIZE_MAX when it does not fit */
size_t nastar_soft_fields_tiled_workspace_bytes(int B, int H, int W);

/* the bytes of the tape of a call: B * (horizon / checkpoint_every + 1) * H * W * 4; 0 when an argument is below 1, SIZE_MAX when the
 * product does not fit */
size_t nastar_soft_fields_tiled_tape_bytes(int B, int H, int W, int horizon, int checkpoint_every);

/* bytes of workspace (device memory, 16-byte aligned) a backward call needs: min(checkpoint_every, horizon) - 1 planes of the segment
 * buffer, and what does not depend on the horizon: the costs in units, V_0, A twice, the fp64 sums and the per-map flags (six planes' worth
 * of 4 B per cell and a little more); 0 when an argument is below 1, SIZE_MAX when it does not fit */
size_t nastar_soft_fields_tiled_backward_workspace_bytes(int B, int H, int W, int horizon, int checkpoint_every);

/* The arguments of nastar_soft_cost_to_go, then: checkpoint_every (looked at with a tape only, but always >= 1), and workspace /
 * workspace_bytes >= nastar_soft_fields_tiled_workspace_bytes(B, H, W).  Refused before any HIP call, in this order: an invalid
 * neighbor_mask (NASTAR_ERR_UNSUPPORTED); a NULL cost / goal / passable / dist_out / status_out / workspace (NASTAR_ERR_NULL); B, H, W,
 * horizon or checkpoint_every < 1, or a tau that is not finite and positive (NASTAR_ERR_BAD_SHAPE); H*W above
 * nastar_soft_fields_tiled_max_cells() or more than 2^24 tiles in the batch (NASTAR_ERR_UNSUPPORTED); a tape or a workspace that is too
 * small or misaligned (NASTAR_ERR_WORKSPACE).  After a failed launch nothing more is enqueued and NASTAR_ERR_HIP is returned. */
int nastar_soft_cost_to_go_tiled(const float* cost, const float* goal, const float* passable, int B, int H, int W, unsigned neighbor_mask,
                                 double tau, int horizon, float* dist_out, float* policy_out, int32_t* status_out, void* tape,
                                 size_t tape_bytes, int checkpoint_every, void* workspace, size_t workspace_bytes, void* stream);

/* the same call with sweeps_per_launch in 1 .. S instead of S (otherwise NASTAR_ERR_BAD_SHAPE, with the shape): the same bits in more
 * launches.  For probes and tests, as launches_per_batch of nastar_cost_to_go_tiled_batched is: not a stable interface. */
int nastar_soft_cost_to_go_tiled_with_sweeps(const float* cost, const float* goal, const float* passable, int B, int H, int W,
                                             unsigned neighbor_mask, double tau, int horizon, float* dist_out, float* policy_out,
                                             int32_t* status_out, void* tape, size_t tape_bytes, int checkpoint_every, void* workspace,
                                             size_t workspace_bytes, int sweeps_per_launch, void* stream);

/* cost, goal, passable, neighbor_mask, tau, horizon, checkpoint_every: those of the nastar_soft_cost_to_go_tiled call that wrote `tape`;
 * grad_dist [B,H,W] fp32, read on the cells live at K only; grad_cost_out [B,H,W] fp32; status_out [B] int32 (NASTAR_OK, or
 * NASTAR_ERR_BAD_COST with an all-zero grad_cost); workspace_bytes >= nastar_soft_fields_tiled_backward_workspace_bytes(B, H, W, horizon,
 * checkpoint_every).  Refused before any HIP call, in this order: an invalid neighbor_mask (NASTAR_ERR_UNSUPPORTED); a NULL cost / goal /
 * passable / tape / grad_dist / grad_cost_out / status_out / workspace (NASTAR_ERR_NULL); B, H, W, horizon or checkpoint_every < 1, or a
 * tau that is not finite and positive (NASTAR_ERR_BAD_SHAPE); H*W above nastar_soft_fields_tiled_max_cells() or more than 2^24 tiles in
 * the batch (NASTAR_ERR_UNSUPPORTED); a tape or a workspace that is too small or misaligned (NASTAR_ERR_WORKSPACE). */
int nastar_soft_fields_backward_tiled(const float* cost, const float* goal, const float* passable, const void* tape, size_t tape_bytes,
                                      int checkpoint_every, const float* grad_dist, int B, int H, int W, unsigned neighbor_mask, double tau,
                                      int horizon, float* grad_cost_out, int32_t* status_out, void* workspace, size_t workspace_bytes,
                                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NASTAR_SOFT_FIELDS_TILED_H_ */
