/* nastar_levels.h -- a search launch that places its maps by their LEVELS itself: an extension BESIDE include/nastar.h (libnastar_hip.so
 * exports both; nothing in nastar.h changes and NASTAR_VERSION stays what it is -- ask nastar_levels_abi()).
 *
 * A launch lasts as long as its longest search, and a long search that starts first runs at lone-wavefront speed (nastar.h:
 * nastar_forward_ordered).  A fresh batch that carries levels -- levels[b] = any non-negative number that grows with the expected length of
 * map b's search, e.g. the optimal distance of its start cell -- gets its placement from nastar_placement_from_levels: one more launch, one
 * more array, in front of the search.  The entry point below needs neither: every workgroup computes which map it searches from 64 of the
 * levels, alone.
 *
 *   nblk = ceil(B / 64).  Block j holds the maps j, j + nblk, j + 2 nblk, ... below B (at most 64).  Workgroup i takes block j = i % nblk and
 *   rank r = i / nblk: it searches the member of block j with exactly r members ahead of it -- larger clamp(level, 0, 4095) first, the lower
 *   map index first among equals.
 *
 * A permutation of 0..B-1 for every B and whatever `levels` holds (nothing to check, nothing out of bounds); workgroups [0, nblk) search the
 * longest map of every block, [nblk, 2 nblk) the second longest, ...  Not the exact global rank -- the launch time does not need it.
 * Outputs are indexed by MAP and do not depend on the placement.
 */
#ifndef NASTAR_LEVELS_H_
#define NASTAR_LEVELS_H_

#include "nastar.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NASTAR_LEVELS_ABI 1

/* 1: the rule described above */
int nastar_levels_abi(void);

/* nastar_forward_ex with `levels` ([B] int32, device) in place of order / order_out; no workspace is needed for the placement.  Validation,
 * packed_out, status_summary and completion_counter as in nastar_forward_ex.  Refused before any HIP call: levels NULL (NASTAR_ERR_NULL); a
 * launch without a kernel that ranks in the launch -- nastar_levels_in_launch() == 0 -- or map pointers that are not 16-byte aligned
 * (NASTAR_ERR_UNSUPPORTED): sort with nastar_placement_from_levels and call nastar_forward_ex instead. */
int nastar_forward_levels(const float* cost, const float* start, const float* goal, const float* passable, int B, int H, int W, double g_ratio,
                          int max_iters, float* histories_out, int64_t* paths_out, int32_t* sel_log_out, int32_t* iters_out, int32_t* status_out,
                          uint8_t* packed_out, void* workspace, size_t workspace_bytes, int flags, const int32_t* levels,
                          int32_t* status_summary, int32_t* completion_counter, void* stream);

/* 1 / 0: would nastar_forward_levels rank in the launch?  Host only, no HIP call.  1 for 16x16, 32x32 and 64x64 maps searched by the
 * hand-scheduled streams without a selection log; 0 under NASTAR_FLAG_UNIT_COST, in lock-step mode, for every other size (compiled loops,
 * maps outside LDS) and with want_log != 0.  (Neighbour masks, heuristic maps and multi-source searches have entry points of their own.) */
int nastar_levels_in_launch(int H, int W, int flags, int want_log);

/* order_out[i] ([B] int32, device) = the map that workgroup i of a nastar_forward_levels launch with these levels searches: B workgroups
 * that evaluate the same device function.  For tests, and for a caller who wants to see the placement. */
int nastar_placement_slots(const int32_t* levels, int B, int32_t* order_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NASTAR_LEVELS_H_ */
