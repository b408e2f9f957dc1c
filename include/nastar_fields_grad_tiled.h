/* nastar_fields_grad_tiled.h -- the gradient of the cost-to-go field with respect to the cost maps (include/nastar_fields_grad.h) for maps of
 * up to nastar_fields_grad_tiled_max_cells() cells: a TILED subtree sum.  A ninth header BESIDE the others: nothing in them changes,
 * NASTAR_VERSION stays what it is -- ask nastar_fields_grad_tiled_abi().
 *
 * Definition: nothing new.  readable, successor, live, A(v) = G(v) + A(c_0) + A(c_1) + ..., grad_cost = fl32(A) on live cells and exactly
 * 0.0f elsewhere, the row-major order of the children, G read on live cells only, fp64 accumulation rounded once at the store and
 * NASTAR_ERR_PLATEAU (11) are those of nastar_fields_grad.h, word for word; on the sizes both take, the results are the same BITS (DESIGN.md
 * section 2, item 6h).  `dist` is what nastar_cost_to_go or nastar_cost_to_go_tiled wrote.
 *
 * What differs is how the sums are reached.  The fp64 accumulator A lives in the workspace (8 B per cell, and one successor byte); the map is
 * cut into the tiles of nastar_fields_tiled.h; a ROUND is one launch in which every tile that is marked active loads itself and a one-cell
 * halo, recomputes its cells to the local fixed point in LDS, stores the cells whose bits changed and marks, for the next round, the
 * adjacent tiles that read one of them.  Nothing is handed from one workgroup to another inside a launch: no grid barrier, no spin on a
 * flag, no workgroup that waits for another, no floating-point atomic; a value crosses a tile border at a kernel boundary.  Rounds are
 * enqueued in batches, after each batch the host reads one word per map and stops when no map marked a tile in the batch's last round -- at
 * the latest after max_rounds rounds (H*W + 1 bounds the count for every input: every round with an active tile makes one more cell final).
 *
 * One addition to the statuses: a map that still has an active tile when max_rounds is reached gets NASTAR_ERR_NO_CONVERGENCE (10) and an
 * ALL-ZERO grad_cost -- a partial subtree sum is a bound of nothing.  Precedence: plateau, then no convergence, then NASTAR_OK.
 *
 * nastar_fields_backward_tiled BLOCKS (it synchronises `stream` after every batch) and therefore cannot be captured into a hipGraph.
 */
#ifndef NASTAR_FIELDS_GRAD_TILED_H_
#define NASTAR_FIELDS_GRAD_TILED_H_

#include "nastar_fields_grad.h"
#include "nastar_fields_tiled.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NASTAR_FIELDS_GRAD_TILED_ABI 1

/* 1: the definition of nastar_fields_grad.h, computed as described above */
int nastar_fields_grad_tiled_abi(void);

/* the largest H*W nastar_fields_backward_tiled takes: 1179648, the limit of nastar_cost_to_go_tiled */
int nastar_fields_grad_tiled_max_cells(void);

/* bytes of workspace (device memory, 8-byte aligned) a call on B maps of H x W needs; 0 for arguments the call refuses */
size_t nastar_fields_backward_tiled_workspace_bytes(int B, int H, int W);

/* dist, goal, passable, grad_dist: [B,H,W] fp32, device; grad_cost_out [B,H,W] fp32; status_out [B] int32; visits_out: [B] int32 on the
 * device or NULL, the number of (tile, round) pairs in which a tile of the map was recomputed.  max_rounds: 0 = the bound H*W + 1.
 * rounds_out: HOST int or NULL, the number of rounds in which some tile was active.  Refused before any HIP call, in this order: an invalid
 * neighbor_mask (NASTAR_ERR_UNSUPPORTED), a NULL dist / goal / passable / grad_dist / grad_cost_out / status_out / workspace
 * (NASTAR_ERR_NULL), B, H or W < 1 or max_rounds < 0 (NASTAR_ERR_BAD_SHAPE), H*W above nastar_fields_grad_tiled_max_cells() or more than
 * 2^24 tiles in the batch (NASTAR_ERR_UNSUPPORTED), workspace_bytes below nastar_fields_backward_tiled_workspace_bytes or a workspace off an
 * 8-byte boundary (NASTAR_ERR_WORKSPACE).  After a HIP error nothing more is launched and NASTAR_ERR_HIP is returned. */
int nastar_fields_backward_tiled(const float* dist, const float* goal, const float* passable, const float* grad_dist, int B, int H, int W,
                                 unsigned neighbor_mask, float* grad_cost_out, int32_t* status_out, int32_t* visits_out, void* workspace,
                                 size_t workspace_bytes, long long max_rounds, int* rounds_out, void* stream);

/* the plateau verdict alone: status_out [B] = NASTAR_ERR_PLATEAU for a map with a live cell that has no successor, NASTAR_OK otherwise.  The
 * first launch of nastar_fields_backward_tiled and a status write: no round, no host read -- it does not block.  Same workspace, same
 * refusals in the same order (NULL: dist / goal / passable / status_out / workspace). */
int nastar_fields_backward_tiled_status(const float* dist, const float* goal, const float* passable, int B, int H, int W,
                                        unsigned neighbor_mask, int32_t* status_out, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NASTAR_FIELDS_GRAD_TILED_H_ */
