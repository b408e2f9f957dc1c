/* nastar_ticket.h -- one entry point for a search launch AND the proof that its batch is solvable (include/nastar_verdict.h), with the proof
 * ordered behind the search launch's own START instead of an event in front of it: an extension BESIDE include/nastar.h (libnastar_hip.so
 * exports both; nothing in nastar.h, nastar_levels.h or nastar_verdict.h changes -- ask nastar_ticket_abi()).
 *
 * nastar_solvable_proof orders its side stream behind the caller's stream with an event, recorded in front of the search launch it
 * accompanies.  A loop of checked searches then queues `marker, search, marker, search, ...` on the caller's stream, and every marker is a
 * barrier of its own between two launches.  The marker only has to say "the maps are final" -- and the search launch behind it says the same:
 * it is dispatched behind a barrier, so none of its workgroups starts before everything queued earlier on the stream is complete.  Here
 * workgroup 0 of the search launch stores a TICKET to a word of signal memory ahead of its first return, and the side stream waits for that
 * value with a stream memory operation (hipStreamWaitValue64: the command processor waits, no wavefront spins).  The caller's stream holds
 * `search, search, ...`.
 *
 * Tickets are the numbers 1, 2, 3, ... of one device, and ticket n lives in slot n % NASTAR_TICKET_RING of a ring allocated at the first
 * call.  The proofs run in issue order on ONE side stream, so the wait of a slot's next user is reached only after its earlier user's proof
 * is over; and the host hands out a slot again only once it has SEEN that earlier proof over (an event per half ring, queried -- never
 * waited for), so the store of an earlier ticket can never land on top of a later one, whatever streams the callers use.  A call that
 * finds its half of the ring still busy takes the event order, as does every call for which the ticket order is not available:
 *   - the device does not report hipDeviceAttributeCanUseStreamWaitValue, or the ring could not be allocated;
 *   - `stream` is capturing;
 *   - the search launch of this shape carries no ticket (the unit-cost layout, maps outside LDS);
 *   - the environment holds NASTAR_PROOF_ORDER=event (read once, at the first call: for A/B measurements of one library).
 * What the ticket order costs: the command processor's wait for a value is slower than an event's barrier, so the proof starts a few
 * microseconds later than in the event order and its verdict arrives later (measured: DESIGN.md 4.1, profiles/proof_ticket.json).  A loop of
 * large launches gains; a caller with much host work per step may prefer NASTAR_PROOF_ORDER=event.
 * No wait is left unsatisfied: it is enqueued only after the search launch was accepted, and if anything fails behind it the host stores
 * the ticket itself.
 */
#ifndef NASTAR_TICKET_H_
#define NASTAR_TICKET_H_

#include "nastar.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NASTAR_TICKET_ABI 1
#define NASTAR_TICKET_RING 32 /* slots of the ring: tickets in flight before a call falls back to the event order */

/* 1: the rule described above */
int nastar_ticket_abi(void);

/* 1 / 0: would a call on the current device and a stream that is not capturing order its proof by ticket?  (Creates the side stream and the
 * ring when they do not exist yet.)  0 under NASTAR_PROOF_ORDER=event. */
int nastar_proof_ticket_available(void);

/* how many proofs of the current device were ordered by ticket / by event through nastar_forward_proved so far (either may be NULL): for
 * tests and measurements */
int nastar_proof_order_counts(long long* by_ticket, long long* by_event);

/* nastar_forward_ex -- or, with `levels` non-NULL, nastar_forward_levels (order and order_out are then ignored) -- and nastar_solvable_proof
 * of the same maps in ONE call.  Returns what the search launch returned.  *proof_rc (host, required) = NASTAR_OK when the proof was
 * launched, else why not: the refusals of nastar_solvable_proof (then the search is launched alone), NASTAR_ERR_UNSUPPORTED after a search
 * launch that was refused or failed (no proof is launched then and none is pending), or NASTAR_ERR_HIP.
 *   proved_out, proof_word, proof_counter   as proved_out, word and counter of nastar_solvable_proof
 * The proof runs on the side stream that nastar_solvable_proof_sync() waits for. */
int nastar_forward_proved(const float* cost, const float* start, const float* goal, const float* passable, int B, int H, int W, double g_ratio,
                          int max_iters, float* histories_out, int64_t* paths_out, int32_t* sel_log_out, int32_t* iters_out, int32_t* status_out,
                          uint8_t* packed_out, void* workspace, size_t workspace_bytes, int flags, const int32_t* order, int32_t* order_out,
                          int32_t* status_summary, int32_t* completion_counter, const int32_t* levels, int32_t* proved_out, int32_t* proof_word,
                          int32_t* proof_counter, int* proof_rc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NASTAR_TICKET_H_ */
