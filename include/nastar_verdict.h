/* nastar_verdict.h -- a proof that every map of a batch is SOLVABLE, computed beside the search launch: an extension BESIDE include/nastar.h
 * (libnastar_hip.so exports both; nothing in nastar.h changes and NASTAR_VERSION stays what it is -- ask nastar_verdict_abi()).
 *
 * A checked search call returns once the launch's completion flag is up, i.e. when the LONGEST search of the batch is over (nastar.h:
 * completion_counter), and nothing the host does for the next call can overlap the device.  For a Moore-8 search without heuristic maps,
 * with g_ratio in [0.5, 0.75] and a budget of at least H * W steps, "every map ends with status 0 and no summary cell" is a property of the
 * inputs alone: the goal is reachable from the start over passable cells.  That is a bit-parallel flood fill, which a caller can wait for
 * instead of the searches.  Alone on the device it takes a few microseconds; beside the search launch it accompanies it issues only in the
 * slots the searching wavefronts leave and takes a good part of that launch's duration (measured: profiles/lean_proof.json).
 *
 *   proved[b] = 1 only if ALL of
 *     (a) the start map and the goal map each hold a non-zero cell (the cell taken is the one with the highest index, as the search takes it);
 *     (b) every cost value c of the map satisfies 0 <= c <= 61440 / (H * W) -- 60 on a 32x32 map, 15 on a 64x64 map (NaN fails, -0.0
 *         passes).  The lower bound is the search kernels' own test for the raw-key instruction stream.  The upper bound keeps every
 *         accumulated g below 2^16, where fp32 still orders the goal's key strictly below the key of every cell its expansion would open
 *         (the fixed-point test behind NASTAR_SUMMARY_COUPLED) -- for g_ratio in [0.5, 0.75]: the bound does not cover a larger g_ratio,
 *         and a caller must not rely on the proof there;
 *     (c) the goal cell is in the closure of the start cell under "step to one of the 8 neighbours whose passable value is non-zero" (the
 *         start cell itself need not be passable; start == goal is reachable).
 *   Anything else is 0: a map that is not proved is simply left to the search's own verdict.
 *
 * Why proved[b] implies status 0 for the launches named above: a closed cell never reopens, every step closes a new cell while the open list
 * is not empty, the open list cannot run empty before a reachable goal is selected, H * W steps cannot be exhausted, and with costs in
 * the range of (b) and g_ratio in [0.5, 0.75] a finished map is at a fixed point of the reference's batch loop in fp32 as well as in exact
 * arithmetic (the error analysis is in csrc/nastar_verdict.hip.h).
 */
#ifndef NASTAR_VERDICT_H_
#define NASTAR_VERDICT_H_

#include "nastar.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NASTAR_VERDICT_ABI 1
#define NASTAR_PROOF_ALL 1  /* the terminal word: every map of the batch is proved */
#define NASTAR_PROOF_SOME 2 /* the terminal word: the launch is over, at least one map is not proved */

/* 1: the rule described above */
int nastar_verdict_abi(void);

/* 1 / 0: is there a proof kernel for H x W maps?  Host only, no HIP call.  1 for 32x32 and 64x64. */
int nastar_solvable_proof_supported(int H, int W);

/* Launch the proof of one batch ([B, H, W] fp32 maps on the device, 16-byte aligned; passable may be the cost pointer itself and is then
 * read once).  The launch goes to a non-blocking side stream that the library owns (one per device, created at the first call), behind an
 * event recorded on `stream` in this call: it sees the inputs as the work queued on `stream` SO FAR leaves them and does not wait for
 * anything queued on `stream` afterwards -- call it BEFORE the search launch it accompanies.
 *   proved_out  optional [B] int32, device: proved[b]
 *   word        one int32 the device can write and the host can read (pinned host memory), 0 on entry: becomes NASTAR_PROOF_ALL or
 *               NASTAR_PROOF_SOME when the last map is done -- always, so a host that sees it non-zero also knows that the launch no
 *               longer reads its inputs
 *   counter     one int32 device cell, 0 on entry, 0 again when `word` is written
 * The launch uses no LDS and at most one wavefront per SIMD.  Refused before any HIP call: a NULL cost / start / goal / passable / word /
 * counter (NASTAR_ERR_NULL), B, H or W < 1 (NASTAR_ERR_BAD_SHAPE), a size without a kernel or map pointers that are not 16-byte aligned
 * (NASTAR_ERR_UNSUPPORTED). */
int nastar_solvable_proof(const float* cost, const float* start, const float* goal, const float* passable, int B, int H, int W,
                          int32_t* proved_out, int32_t* word, int32_t* counter, void* stream);

/* wait for everything queued on the current device's side stream (nothing to wait for before the first launch) */
int nastar_solvable_proof_sync(void);

#ifdef __cplusplus
}
#endif
#endif /* NASTAR_VERDICT_H_ */
