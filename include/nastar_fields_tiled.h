/* nastar_fields_tiled.h -- the cost-to-go field of include/nastar_fields.h for maps of up to nastar_fields_tiled_max_cells() cells (the search's
 * own limit): a TILED relaxation of the same definition.  A sixth header BESIDE nastar.h and nastar_fields.h: nothing in either changes.
 *
 * Definition, moves, policy rule and status codes are those of nastar_fields.h, word for word; the results are the same BITS (DESIGN.md
 * section 2, item 6f).  What differs is how the fixed point is reached.  The working field lives in dist_out itself; the map is cut into tiles
 * of nastar_fields_tile() cells; a ROUND is one launch in which every tile that is marked active loads itself and a one-cell halo, relaxes
 * to its local fixed point in LDS, stores the cells it lowered and marks, for the next round, the adjacent tiles whose halo holds one of
 * them.  Nothing is handed from one workgroup to another inside a launch: no grid barrier, no spin on a flag, no workgroup that waits for
 * another; a value crosses a tile border at a kernel boundary.  Rounds are enqueued in batches, after each batch the host reads one word per
 * map and stops when no map marked a tile in the batch's last round -- at the latest after max_rounds rounds (H*W + 1 bounds the count
 * for every accepted input: every round with an active tile makes one more cell final).
 *
 * The call BLOCKS (it synchronises `stream` after every batch) and therefore cannot be captured into a hipGraph.
 */
#ifndef NASTAR_FIELDS_TILED_H_
#define NASTAR_FIELDS_TILED_H_

#include "nastar_fields.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NASTAR_FIELDS_TILED_ABI 1

/* 1: the definition of nastar_fields.h, computed as described above */
int nastar_fields_tiled_abi(void);

/* the largest H*W nastar_cost_to_go_tiled takes: 1179648, the limit of the search entry points */
int nastar_fields_tiled_max_cells(void);

/* the interior of one tile, rows and columns (tests derive their shapes from it) */
int nastar_fields_tile(int* th, int* tw);

/* bytes of workspace (device memory, 4-byte aligned) a call on B maps of H x W needs; 0 for arguments the call refuses */
size_t nastar_cost_to_go_tiled_workspace_bytes(int B, int H, int W);

/* cost, goal, passable, dist_out, policy_out (may be NULL), status_out: as nastar_cost_to_go.  visits_out: [B] int32 on the device or NULL,
 * the number of (tile, round) pairs in which a tile of the map was relaxed.  max_rounds: 0 = the bound H*W + 1; a map that still has an
 * active tile after max_rounds rounds gets NASTAR_ERR_NO_CONVERGENCE and a dist_out that is an upper bound of its field, finite only where
 * the field is.  rounds_out: HOST int or NULL, the number of rounds in which some tile was active.  Refused before any HIP call: an
 * invalid neighbor_mask (NASTAR_ERR_UNSUPPORTED), a NULL cost / goal / passable / dist_out / status_out / workspace (NASTAR_ERR_NULL), B, H,
 * W < 1 or max_rounds < 0 (NASTAR_ERR_BAD_SHAPE), H*W above nastar_fields_tiled_max_cells() or more than 2^24 tiles in the batch
 * (NASTAR_ERR_UNSUPPORTED), workspace_bytes below nastar_cost_to_go_tiled_workspace_bytes or a workspace off a 4-byte boundary (NASTAR_ERR_WORKSPACE).  After a HIP error nothing
 * more is launched and NASTAR_ERR_HIP is returned. */
int nastar_cost_to_go_tiled(const float* cost, const float* goal, const float* passable, int B, int H, int W, unsigned neighbor_mask,
                            float* dist_out, float* policy_out, int32_t* status_out, int32_t* visits_out, void* workspace, size_t workspace_bytes,
                            long long max_rounds, int* rounds_out, void* stream);

/* nastar_cost_to_go_tiled with the number of rounds enqueued between two reads of the host chosen by the caller (launches_per_batch >= 1;
 * 0 = the library's choice).  For probes ONLY: the results do not depend on it, and this entry point is not a stable part of the interface --
 * it may change or go with the next NASTAR_FIELDS_TILED_ABI. */
int nastar_cost_to_go_tiled_batched(const float* cost, const float* goal, const float* passable, int B, int H, int W, unsigned neighbor_mask,
                                    float* dist_out, float* policy_out, int32_t* status_out, int32_t* visits_out, void* workspace,
                                    size_t workspace_bytes, long long max_rounds, int launches_per_batch, int* rounds_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NASTAR_FIELDS_TILED_H_ */
