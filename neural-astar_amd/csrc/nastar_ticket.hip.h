// nastar_ticket.hip.h -- host only: what the two translation units behind include/nastar_ticket.h share.  nastar_verdict_capi.hip owns the
// proof's side stream and the ring of tickets; nastar_capi.hip owns the search launch that carries one.  Nothing here crosses the C ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace nastar {

// the arguments of nastar_forward_ex, `levels` (non-null: nastar_forward_levels, then order / order_out are not used), and the ticket: the
// word the launch stores `ticket_value` to when it starts (null: no ticket)
struct TicketedSearch {
    const float *cost, *start, *goal, *passable;
    int B, H, W;
    double g_ratio;
    int max_iters;
    float* histories_out;
    int64_t* paths_out;
    int32_t *sel_log_out, *iters_out, *status_out;
    uint8_t* packed_out;
    void* workspace;
    size_t workspace_bytes;
    int flags;
    const int32_t *order, *levels;
    int32_t *order_out, *status_summary, *completion_counter;
    void* stream;
    unsigned long long* ticket_word;
    unsigned long long ticket_value;
};

// would the search launch of this shape carry a ticket?  Host only, no HIP call: the LDS-resident searches outside the unit-cost layout
// (nastar_forward_compact_kernel and its ranked twin).  Asked BEFORE the launch -- the event order has to be chosen in front of it.
__attribute__((visibility("hidden"))) bool search_carries_ticket(int H, int W, int flags);

// nastar_forward_ex / nastar_forward_levels with the ticket.  *carried: the kernel that was launched stores the ticket (always what
// search_carries_ticket said, unless the call was refused)
__attribute__((visibility("hidden"))) int forward_ticketed(const TicketedSearch& t, bool* carried);

}  // namespace nastar
