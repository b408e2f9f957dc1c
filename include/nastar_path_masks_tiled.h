/* nastar_path_masks_tiled.h -- the exact shortest-path MASK of include/nastar_path_masks.h and its blackbox gradient for maps of up to
 * nastar_path_masks_tiled_max_cells() cells (the search's own limit).  A twelfth header BESIDE the others: nothing in them changes,
 * NASTAR_VERSION stays what it is -- ask nastar_path_masks_tiled_abi().
 *
 * The definition is that of nastar_path_masks.h, word for word: the field, the successor and the route, the mask convention, path_cost_out
 * (the field's own bits at the start), the perturbation w' = fmaxf(fl32(fl32(lambda * g) + w), min_cost) with a NaN staying a NaN, the
 * gradient (y' - y) * fl32(1 / lambda), a zero row for a map whose forward failed and an all-NaN row for a map whose perturbed solve
 * failed.  Where both calls apply (H*W <= nastar_path_masks_max_cells()) the results are the same BITS.  The status is looked at in the
 * same order:
 *       NASTAR_ERR_BAD_SHAPE (1)        start_idx outside [0, H*W)
 *       NASTAR_ERR_BAD_COST (9)         a NaN or a negative cost on a passable cell
 *       NASTAR_ERR_UNSOLVABLE (3)       no goal cell
 *       NASTAR_ERR_NO_CONVERGENCE (10)  the relaxation was cut short by max_rounds (impossible with max_rounds = 0): the field is then
 *                                       only an upper bound, and D(n0) is not looked at
 *       NASTAR_ERR_UNSOLVABLE (3)       D(n0) is not finite (an obstacle, an unreachable start)
 *       NASTAR_ERR_PLATEAU (11)         the chain reaches a cell that is no goal and has no successor (a zero-cost plateau)
 *       NASTAR_OK (0)
 * A failed map has an all-zero mask and a cost of +inf; the other maps of the batch are unaffected.
 *
 * What differs is how the result is reached.  Forward: nastar_cost_to_go_tiled (include/nastar_fields_tiled.h) writes the field into the
 * workspace, 4 bytes per cell, without policy planes; one launch writes the successor of every cell as a byte, the table
 * nastar_field_routes chases, into the workspace as well; then one launch, a workgroup per map, stores the row of zeros, and behind a
 * barrier one lane chases the start along the table and stores a 1 on every route cell; a chase that ends on a plateau walks again and
 * takes its marks back.  Backward: one elementwise launch writes w' into the workspace, the same relaxation runs on w', and the same two
 * launches follow, storing (0 - path_fwd) * inv_lambda everywhere and (1 - path_fwd) * inv_lambda on the perturbed route.  A map that
 * status_fwd skipped IS relaxed all the same -- the tiled relaxation takes whole batches -- but its field is not looked at: its row is
 * zero and its status NASTAR_OK.
 *
 * Both calls BLOCK (the relaxation synchronises `stream` between batches of rounds) and therefore cannot be captured into a hipGraph.
 */
#ifndef NASTAR_PATH_MASKS_TILED_H_
#define NASTAR_PATH_MASKS_TILED_H_

#include "nastar_fields_tiled.h"
#include "nastar_path_masks.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NASTAR_PATH_MASKS_TILED_ABI 1

/* 1: the definition of nastar_path_masks.h, computed as described above */
int nastar_path_masks_tiled_abi(void);

/* the largest H*W both calls take: 1179648, nastar_fields_tiled_max_cells() */
int nastar_path_masks_tiled_max_cells(void);

/* bytes of workspace (device memory, 4-byte aligned) a forward / a backward call on B maps of H x W needs: the field (4 bytes per cell),
 * the relaxation's per-map status and its own workspace, the successor table (1 byte per cell); the backward adds the perturbed costs
 * (4 bytes per cell).  0 for arguments the call refuses */
size_t nastar_path_masks_tiled_workspace_bytes(int B, int H, int W);
size_t nastar_path_masks_tiled_backward_workspace_bytes(int B, int H, int W);

/* cost, goal, passable, start_idx, path_out, path_cost_out (may be NULL), status_out: as nastar_path_masks.  max_rounds: as
 * nastar_cost_to_go_tiled, 0 = the bound H*W + 1; a map cut short gets NASTAR_ERR_NO_CONVERGENCE, an all-zero mask and a cost of +inf.
 * rounds_out: HOST int or NULL, the rounds of the relaxation in which some tile was active.  Refused before any HIP call, in this order:
 * an invalid neighbor_mask (NASTAR_ERR_UNSUPPORTED), a NULL cost / goal / passable / start_idx / path_out / status_out / workspace
 * (NASTAR_ERR_NULL), B, H or W < 1 or max_rounds < 0 (NASTAR_ERR_BAD_SHAPE), H*W above nastar_path_masks_tiled_max_cells() or more than
 * 2^24 tiles in the batch (NASTAR_ERR_UNSUPPORTED), workspace_bytes below nastar_path_masks_tiled_workspace_bytes or a workspace off a
 * 4-byte boundary (NASTAR_ERR_WORKSPACE).  After a HIP error nothing more is launched and NASTAR_ERR_HIP is returned. */
int nastar_path_masks_tiled(const float* cost, const float* goal, const float* passable, const int32_t* start_idx, int B, int H, int W,
                            unsigned neighbor_mask, float* path_out, float* path_cost_out, int32_t* status_out, void* workspace,
                            size_t workspace_bytes, long long max_rounds, int* rounds_out, void* stream);

/* the inputs of nastar_path_masks_tiled; grad_path, path_fwd, status_fwd, lambda, min_cost, grad_cost_out and status_out (may be NULL): as
 * nastar_path_masks_backward.  max_rounds bounds the PERTURBED relaxation: a map cut short is a failed perturbed solve -- an all-NaN row
 * and NASTAR_ERR_NO_CONVERGENCE.  rounds_out: HOST int or NULL, the rounds of that relaxation.  Refused before any HIP call, in this
 * order: an invalid neighbor_mask (NASTAR_ERR_UNSUPPORTED), a NULL cost / goal / passable / start_idx / grad_path / path_fwd / status_fwd /
 * grad_cost_out / workspace (NASTAR_ERR_NULL), B, H or W < 1 or max_rounds < 0 (NASTAR_ERR_BAD_SHAPE), H*W above
 * nastar_path_masks_tiled_max_cells() or more than 2^24 tiles in the batch, then a lambda or min_cost that is not a finite positive number
 * or a lambda whose fp32 reciprocal is not finite (NASTAR_ERR_UNSUPPORTED), workspace_bytes below
 * nastar_path_masks_tiled_backward_workspace_bytes or a workspace off a 4-byte boundary (NASTAR_ERR_WORKSPACE).  After a HIP error
 * nothing more is launched and NASTAR_ERR_HIP is returned. */
int nastar_path_masks_tiled_backward(const float* cost, const float* goal, const float* passable, const int32_t* start_idx,
                                     const float* grad_path, const float* path_fwd, const int32_t* status_fwd, int B, int H, int W,
                                     unsigned neighbor_mask, float lambda, float min_cost, float* grad_cost_out, int32_t* status_out,
                                     void* workspace, size_t workspace_bytes, long long max_rounds, int* rounds_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NASTAR_PATH_MASKS_TILED_H_ */
