/* nastar_soft_policy_tiled.h -- the LOG-POLICY of the entropy-regularised cost-to-go field and the vector-Jacobian product through it
 * (include/nastar_soft_policy.h) for maps of up to nastar_soft_fields_tiled_max_cells() cells: the tiled sweeps and the checkpointed tape of
 * include/nastar_soft_fields_tiled.h.  A seventeenth header BESIDE the others: nothing in them changes, NASTAR_VERSION stays what it is --
 * ask nastar_soft_policy_tiled_abi().
 *
 * Definition: nothing new.  From nastar_soft_policy.h, word for word: the log-policy, Act(n) and where -inf lies; the read rule of the two
 * seeds, gsum, Z and the gather order; A_{K-1} = (the gather) + Z in fp32, in that order; the K = 1 rule (GL is not read and contributes
 * exactly 0.0f); an output linear in the two seeds and exactly 0.0f on a cell that was never live; the fp64 sum over k with one rounding at
 * the store.  From nastar_soft_fields_tiled.h: the tiles and their halo, the prepare launch, the tape with checkpoint_every, the workspace
 * rules, and "only enqueues, reads nothing back".  The cell expressions are the one-workgroup kernels' own, so log_policy and grad_cost are
 * the same BITS as nastar_soft_policy_forward / nastar_soft_policy_backward give on every map both take.
 *
 *   tape       that of nastar_soft_fields_tiled.h (nastar_soft_fields_tiled_tape_bytes): either tiled forward's tape feeds either tiled
 *              backward.
 *   forward    dist, policy, status and the tape are the bits of nastar_soft_cost_to_go_tiled.  log_policy_out is written by the launch
 *              that reaches plane K, from the minimum, the sum and the plane K-1 that launch already holds: no sweep, no plane and no launch
 *              more.
 *   backward   the launches of nastar_soft_fields_backward_tiled, except that step K -- with a grad_log_policy and K >= 2 -- is a launch
 *              that also forms Q(n) = gsum(n) / S_K(n) on its tile and one ring, where n is live at K (read from the costs and plane K, the
 *              tape's final slot), and adds Z in its gather.  Q stays in the workgroup's LDS: the workspace is the field's.  With
 *              grad_log_policy = NULL or K = 1 exactly the launches, and the bits, of nastar_soft_fields_backward_tiled (grad_dist = NULL
 *              read as zeros); with both NULL all +0.0f.  One workgroup owns a cell: no atomics, two calls give the same bits; the result
 *              does not depend on checkpoint_every.
 */
#ifndef NASTAR_SOFT_POLICY_TILED_H_
#define NASTAR_SOFT_POLICY_TILED_H_

#include "nastar_soft_fields_tiled.h"
#include "nastar_soft_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NASTAR_SOFT_POLICY_TILED_ABI 1

/* 1: the definition of nastar_soft_policy.h, computed as described above */
int nastar_soft_policy_tiled_abi(void);

/* The arguments of nastar_soft_cost_to_go_tiled, and log_policy_out [B,8,H,W] fp32 behind policy_out; workspace_bytes >=
 * nastar_soft_fields_tiled_workspace_bytes(B, H, W).  Refused before any HIP call, in this order: an invalid neighbor_mask
 * (NASTAR_ERR_UNSUPPORTED); a NULL cost / goal / passable / dist_out / log_policy_out / status_out / workspace (NASTAR_ERR_NULL; policy_out
 * may be NULL: no policy is written); B, H, W, horizon or checkpoint_every < 1, or a tau that is not finite and positive
 * (NASTAR_ERR_BAD_SHAPE); H*W above nastar_soft_fields_tiled_max_cells() or more than 2^24 tiles in the batch (NASTAR_ERR_UNSUPPORTED); a
 * tape or a workspace that is too small or misaligned (NASTAR_ERR_WORKSPACE).  After a failed launch nothing more is enqueued and
 * NASTAR_ERR_HIP is returned. */
int nastar_soft_policy_forward_tiled(const float* cost, const float* goal, const float* passable, int B, int H, int W, unsigned neighbor_mask,
                                     double tau, int horizon, float* dist_out, float* policy_out, float* log_policy_out, int32_t* status_out,
                                     void* tape, size_t tape_bytes, int checkpoint_every, void* workspace, size_t workspace_bytes,
                                     void* stream);

/* the same call with sweeps_per_launch in 1 .. S instead of S (otherwise NASTAR_ERR_BAD_SHAPE, with the shape): the same bits in more
 * launches.  For probes and tests, as nastar_soft_cost_to_go_tiled_with_sweeps is: not a stable interface. */
int nastar_soft_policy_forward_tiled_with_sweeps(const float* cost, const float* goal, const float* passable, int B, int H, int W,
                                                 unsigned neighbor_mask, double tau, int horizon, float* dist_out, float* policy_out,
                                                 float* log_policy_out, int32_t* status_out, void* tape, size_t tape_bytes,
                                                 int checkpoint_every, void* workspace, size_t workspace_bytes, int sweeps_per_launch,
                                                 void* stream);

/* bytes of workspace (device memory, 16-byte aligned) a backward call needs: nastar_soft_fields_tiled_backward_workspace_bytes(B, H, W,
 * horizon, checkpoint_every) -- the injected step keeps what it adds in LDS; 0 when an argument is below 1, SIZE_MAX when it does not fit */
size_t nastar_soft_policy_tiled_backward_workspace_bytes(int B, int H, int W, int horizon, int checkpoint_every);

/* The arguments of nastar_soft_fields_backward_tiled, with grad_dist [B,H,W] fp32 or NULL (zeros) and, behind it, grad_log_policy
 * [B,8,H,W] fp32 or NULL (zeros); workspace_bytes >= nastar_soft_policy_tiled_backward_workspace_bytes(B, H, W, horizon,
 * checkpoint_every).  Refused before any HIP call, in this order: an invalid neighbor_mask (NASTAR_ERR_UNSUPPORTED); a NULL cost / goal /
 * passable / tape / grad_cost_out / status_out / workspace (NASTAR_ERR_NULL); B, H, W, horizon or checkpoint_every < 1, or a tau that is
 * not finite and positive (NASTAR_ERR_BAD_SHAPE); H*W above nastar_soft_fields_tiled_max_cells() or more than 2^24 tiles in the batch
 * (NASTAR_ERR_UNSUPPORTED); a tape or a workspace that is too small or misaligned (NASTAR_ERR_WORKSPACE). */
int nastar_soft_policy_backward_tiled(const float* cost, const float* goal, const float* passable, const void* tape, size_t tape_bytes,
                                      int checkpoint_every, const float* grad_dist, const float* grad_log_policy, int B, int H, int W,
                                      unsigned neighbor_mask, double tau, int horizon, float* grad_cost_out, int32_t* status_out,
                                      void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NASTAR_SOFT_POLICY_TILED_H_ */
