// nastar_verdict_capi.hip -- the C ABI of include/nastar_verdict.h: the proof that a batch is solvable, launched beside its search.  A
// translation unit of its own: nothing here touches the search, replay or encoder kernels.  include/nastar_ticket.h lives here too -- the
// entry point that issues the search launch (through csrc/nastar_ticket.hip.h: the launch itself stays in nastar_capi.hip) and orders the
// proof behind that launch's own start.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>

#include "nastar_verdict.hip.h"
#include "nastar_host.hip.h"
#include "nastar_ticket.hip.h"
#include "../../include/nastar_verdict.h"
#include "../../include/nastar_ticket.h"

using namespace nastar;

namespace {

// The ring of tickets (include/nastar_ticket.h).  kRing = 32 slots: a loop of checked searches has one or two proofs in flight (the host
// returns on each proof's word), a pipelined caller a handful; a ring is exhausted only by a caller that issues kRing / 2 calls while the
// device is still busy with the proofs of the half ring before -- that call takes the event order, nothing waits.  Every slot is an
// allocation of its own because signal memory comes in single 8-byte words.  The 64-bit form: tickets count up from 1 for the life of the
// library and never wrap, so "the slot holds exactly n" can only mean that launch n has started (0, the initial content, is no ticket).
constexpr int kRing = NASTAR_TICKET_RING, kHalf = kRing / 2;
static_assert(kRing >= 2 && kRing % 2 == 0, "the ring is handed out in two halves");
// the side stream of one device, the event that orders it behind the caller's stream, and the grid (one wavefront per SIMD); made at the
// first launch on that device, kept for the life of the library.  `mutex` serialises what is enqueued on the side stream of THIS device (the
// event is shared, and tickets must be handed out in the order their proofs reach the stream); calls on other devices do not wait for it.
struct ProofLane {
    std::mutex mutex;
    hipStream_t stream = nullptr;
    hipEvent_t event = nullptr;
    int max_grid = 0;
    int ticket_state = 0;                         // 0: not asked yet, 1: the ticket order is available, -1: it is not (any more)
    unsigned long long* ring[kRing] = {};
    hipEvent_t half_done[2] = {nullptr, nullptr};  // recorded on `stream` behind the proof of a half's LAST ticket
    bool half_recorded[2] = {false, false};
    unsigned long long next_ticket = 1;
    long long by_ticket = 0, by_event = 0;
};
constexpr int kMaxDevices = 64;
ProofLane g_lanes[kMaxDevices];

// the current device's lane, LOCKED (`lock` owns its mutex on success), created at the first call
int proof_lane(ProofLane** out, std::unique_lock<std::mutex>& lock)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_fail(e, "hipGetDevice");
    if (dev < 0 || dev >= kMaxDevices) return NASTAR_ERR_UNSUPPORTED;
    ProofLane& l = g_lanes[dev];
    lock = std::unique_lock<std::mutex>(l.mutex);
    if (l.stream == nullptr) {
        int cus = 0;
        if ((e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return hip_fail(e, "hipDeviceGetAttribute");
        // The event only orders the side stream behind the caller's stream ON THIS DEVICE: nobody synchronises with it from the host or asks
        // it for a time.  Recorded with the default flags, its marker packet sits between two consecutive search launches of the caller's
        // stream and performs a system-scope release there (L2 written back and invalidated for the host) -- 2.4 us per checked step,
        // for a consumer that is a kernel of the same device.  hipEventDisableSystemFence leaves the marker as the plain barrier it needs to
        // be: what earlier kernels of the stream wrote is released at device scope by those kernels' own ends, and the proof kernel begins
        // with its own acquire.  (hipEventReleaseToDevice was measured too: no different from the default.  DESIGN 4.1 "The gap", profiles/writethrough_outputs.json)
        hipEvent_t ev = nullptr;
        if ((e = hipEventCreateWithFlags(&ev, hipEventDisableTiming | hipEventDisableSystemFence)) != hipSuccess) return hip_fail(e, "hipEventCreateWithFlags");
        hipStream_t s = nullptr;
        if ((e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking)) != hipSuccess) {
            (void)hipEventDestroy(ev);
            return hip_fail(e, "hipStreamCreateWithFlags");
        }
        l.max_grid = 4 * kProofWavesPerSimd * (cus > 0 ? cus : 1);  // 4 SIMDs per CU
        l.event = ev;
        l.stream = s;
    }
    *out = &l;
    return NASTAR_OK;
}

// NASTAR_PROOF_ORDER=event, read once: nastar_forward_proved never orders by ticket (A/B measurements of one library)
bool event_order_forced()
{
    static const bool forced = [] {
        const char* v = getenv("NASTAR_PROOF_ORDER");
        return v != nullptr && strcmp(v, "event") == 0;
    }();
    return forced;
}

// is the ticket order available on this lane's device?  Decided once: the attribute, then the ring and the two events.  A failure frees
// what was made and leaves the lane on the event order for good.
bool ticket_ready(ProofLane& l)
{
    if (l.ticket_state != 0) return l.ticket_state > 0;
    l.ticket_state = -1;
    if (event_order_forced()) return false;
    int dev = 0, can = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, dev) != hipSuccess || can != 1) {
        (void)hipGetLastError();
        return false;
    }
    bool ok = true;
    for (int i = 0; i < kRing && ok; ++i) {
        void* p = nullptr;
        ok = hipExtMallocWithFlags(&p, sizeof(unsigned long long), hipMallocSignalMemory) == hipSuccess && p != nullptr;
        if (ok) {
            l.ring[i] = static_cast<unsigned long long*>(p);
            __atomic_store_n(l.ring[i], 0ull, __ATOMIC_RELAXED);
        }
    }
    for (int h = 0; h < 2 && ok; ++h) ok = hipEventCreateWithFlags(&l.half_done[h], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        for (int i = 0; i < kRing; ++i)
            if (l.ring[i]) { (void)hipFree(l.ring[i]); l.ring[i] = nullptr; }
        for (int h = 0; h < 2; ++h)
            if (l.half_done[h]) { (void)hipEventDestroy(l.half_done[h]); l.half_done[h] = nullptr; }
        return false;
    }
    l.ticket_state = 1;
    return true;
}

// may ticket n be handed out?  Only the FIRST ticket of a half ring asks: the proofs of that half's earlier tickets (n - kRing ...) must be
// over -- the event behind the last of them is queried, never waited for.  (An earlier proof that is over has seen its search launch's
// store, so no store to these slots is still to come.)
bool half_free(ProofLane& l, unsigned long long n)
{
    if (n % kHalf != 0) return true;
    const int h = (int)((n / kHalf) & 1);
    if (!l.half_recorded[h]) return true;
    const hipError_t e = hipEventQuery(l.half_done[h]);
    if (e == hipSuccess) {
        l.half_recorded[h] = false;
        return true;
    }
    if (e != hipErrorNotReady) (void)hipGetLastError();
    return false;
}

int launch_proof(const ProofLane& l, const float* cost, const float* start, const float* goal, const float* passable, int B, int W, int32_t* proved_out,
                 int32_t* word, int32_t* counter)
{
    const int mpw = 64 / W, ngroups = (B + mpw - 1) / mpw;
    const unsigned grid = (unsigned)(ngroups < l.max_grid ? ngroups : l.max_grid);
    if (W == 32) return launch(nastar_solvable_proof_kernel<5>, (int)grid, 0, l.stream, cost, start, goal, passable, B, proved_out, word, counter);
    return launch(nastar_solvable_proof_kernel<6>, (int)grid, 0, l.stream, cost, start, goal, passable, B, proved_out, word, counter);
}

}  // namespace

extern "C" {

int nastar_verdict_abi(void) { return NASTAR_VERDICT_ABI; }

int nastar_solvable_proof_supported(int H, int W) { return (H == W && (W == 32 || W == 64)) ? 1 : 0; }

int nastar_solvable_proof(const float* cost, const float* start, const float* goal, const float* passable, int B, int H, int W,
                          int32_t* proved_out, int32_t* word, int32_t* counter, void* stream)
{
    if (!cost || !start || !goal || !passable || !word || !counter) return NASTAR_ERR_NULL;
    if (B < 1 || H < 1 || W < 1) return NASTAR_ERR_BAD_SHAPE;
    if (!nastar_solvable_proof_supported(H, W)) return NASTAR_ERR_UNSUPPORTED;
    if (!aligned16(cost) || !aligned16(start) || !aligned16(goal) || !aligned16(passable)) return NASTAR_ERR_UNSUPPORTED;
    std::unique_lock<std::mutex> lock;
    ProofLane* l = nullptr;
    int rc = proof_lane(&l, lock);
    if (rc) return rc;
    hipError_t e = hipEventRecord(l->event, reinterpret_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "hipEventRecord");
    if ((e = hipStreamWaitEvent(l->stream, l->event, 0)) != hipSuccess) return hip_fail(e, "hipStreamWaitEvent");
    return launch_proof(*l, cost, start, goal, passable, B, W, proved_out, word, counter);
}

int nastar_solvable_proof_sync(void)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_fail(e, "hipGetDevice");
    if (dev < 0 || dev >= kMaxDevices) return NASTAR_OK;
    hipStream_t s = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_lanes[dev].mutex);
        s = g_lanes[dev].stream;
    }
    if (s == nullptr) return NASTAR_OK;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
    return NASTAR_OK;
}

// ---- include/nastar_ticket.h ----------------------------------------------------------------------------------------------------------------
int nastar_ticket_abi(void) { return NASTAR_TICKET_ABI; }

int nastar_proof_ticket_available(void)
{
    std::unique_lock<std::mutex> lock;
    ProofLane* l = nullptr;
    if (proof_lane(&l, lock)) return 0;
    return ticket_ready(*l) ? 1 : 0;
}

int nastar_proof_order_counts(long long* by_ticket, long long* by_event)
{
    std::unique_lock<std::mutex> lock;
    ProofLane* l = nullptr;
    const int rc = proof_lane(&l, lock);
    if (rc) return rc;
    if (by_ticket) *by_ticket = l->by_ticket;
    if (by_event) *by_event = l->by_event;
    return NASTAR_OK;
}

int nastar_forward_proved(const float* cost, const float* start, const float* goal, const float* passable, int B, int H, int W, double g_ratio,
                          int max_iters, float* histories_out, int64_t* paths_out, int32_t* sel_log_out, int32_t* iters_out, int32_t* status_out,
                          uint8_t* packed_out, void* workspace, size_t workspace_bytes, int flags, const int32_t* order, int32_t* order_out,
                          int32_t* status_summary, int32_t* completion_counter, const int32_t* levels, int32_t* proved_out, int32_t* proof_word,
                          int32_t* proof_counter, int* proof_rc, void* stream)
{
    if (!proof_rc) return NASTAR_ERR_NULL;
    TicketedSearch t{cost, start, goal, passable, B, H, W, g_ratio, max_iters, histories_out, paths_out, sel_log_out, iters_out, status_out, packed_out,
                     workspace, workspace_bytes, flags, order, levels, order_out, status_summary, completion_counter, stream, nullptr, 0};
    bool carried = false;
    // the refusals of nastar_solvable_proof, in its order: the search then goes out alone
    int prc = NASTAR_OK;
    if (!cost || !start || !goal || !passable || !proof_word || !proof_counter) prc = NASTAR_ERR_NULL;
    else if (B < 1 || H < 1 || W < 1) prc = NASTAR_ERR_BAD_SHAPE;
    else if (!nastar_solvable_proof_supported(H, W) || !aligned16(cost) || !aligned16(start) || !aligned16(goal) || !aligned16(passable))
        prc = NASTAR_ERR_UNSUPPORTED;
    std::unique_lock<std::mutex> lock;  // this device's lane, held across both launches: tickets are handed out in the order the proofs reach the side stream
    ProofLane* l = nullptr;
    if (prc == NASTAR_OK) prc = proof_lane(&l, lock);
    if (prc != NASTAR_OK) {
        *proof_rc = prc;
        if (lock.owns_lock()) lock.unlock();
        return forward_ticketed(t, &carried);
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipError_t e;
    bool by_ticket = search_carries_ticket(H, W, flags) && ticket_ready(*l);
    if (by_ticket) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusActive;  // (a query that fails answers "capturing": the event order)
        if (hipStreamIsCapturing(s, &cs) != hipSuccess) {
            (void)hipGetLastError();
            cs = hipStreamCaptureStatusActive;
        }
        by_ticket = cs == hipStreamCaptureStatusNone && half_free(*l, l->next_ticket);
    }
    *proof_rc = NASTAR_ERR_UNSUPPORTED;  // (what stands when the search launch below is refused)
    if (!by_ticket) {
        // the event order of nastar_solvable_proof, with the proof's launch moved behind the search's: recorded in front of the search launch,
        // waited for only once that launch has been accepted -- a refused search leaves nothing pending
        if ((e = hipEventRecord(l->event, s)) != hipSuccess) {
            *proof_rc = hip_fail(e, "hipEventRecord");
            return forward_ticketed(t, &carried);
        }
        const int rc = forward_ticketed(t, &carried);
        if (rc) return rc;
        if ((e = hipStreamWaitEvent(l->stream, l->event, 0)) != hipSuccess) *proof_rc = hip_fail(e, "hipStreamWaitEvent");
        else *proof_rc = launch_proof(*l, cost, start, goal, passable, B, W, proved_out, proof_word, proof_counter);
        if (*proof_rc == NASTAR_OK) ++l->by_event;
        return rc;
    }
    // the ticket order.  The number is spent whatever happens below: a launch that was handed it may store it at any later time
    const unsigned long long n = l->next_ticket++;
    unsigned long long* const slot = l->ring[n % kRing];
    t.ticket_word = slot;
    t.ticket_value = n;
    const int rc = forward_ticketed(t, &carried);
    if (rc == NASTAR_OK && carried) {
        // 2. the wait, only now that the launch which satisfies it is in the caller's queue; 3. the proof behind it
        if ((e = hipStreamWaitValue64(l->stream, slot, n, hipStreamWaitValueEq)) != hipSuccess) *proof_rc = hip_fail(e, "hipStreamWaitValue64");
        else {
            *proof_rc = launch_proof(*l, cost, start, goal, passable, B, W, proved_out, proof_word, proof_counter);
            if (*proof_rc != NASTAR_OK) __atomic_store_n(slot, n, __ATOMIC_RELEASE);  // nothing may stay behind an unsatisfied wait
        }
        if (*proof_rc == NASTAR_OK) ++l->by_ticket;
    } else if (rc == NASTAR_OK) {
        // search_carries_ticket() (asked in front of the launch) and the kernel choice of forward_lds disagree: the launch that went out stores
        // no ticket.  Nothing waits for one; the proof is ordered behind an event recorded BEHIND the search launch -- late, never lost
        if ((e = hipEventRecord(l->event, s)) != hipSuccess) *proof_rc = hip_fail(e, "hipEventRecord");
        else if ((e = hipStreamWaitEvent(l->stream, l->event, 0)) != hipSuccess) *proof_rc = hip_fail(e, "hipStreamWaitEvent");
        else *proof_rc = launch_proof(*l, cost, start, goal, passable, B, W, proved_out, proof_word, proof_counter);
        if (*proof_rc == NASTAR_OK) ++l->by_event;
    }
    // "the proof of ticket n is over" is what lets slot n % kRing be handed out again (half_free).  A ticket whose launch may be under way
    // without a proof behind it breaks that chain: this device stays on the event order from here on
    if (carried && (rc != NASTAR_OK || *proof_rc != NASTAR_OK)) l->ticket_state = -1;
    if (n % kHalf == kHalf - 1 && l->ticket_state > 0) {
        const int h = (int)((n / kHalf) & 1);
        if ((e = hipEventRecord(l->half_done[h], l->stream)) == hipSuccess) l->half_recorded[h] = true;
        else {
            (void)hipGetLastError();
            l->ticket_state = -1;
        }
    }
    return rc;
}

}  // extern "C"
