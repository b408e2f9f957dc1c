// nastar_forward_compact_body.inc -- the body of nastar_forward_compact_kernel and nastar_forward_compact_masked_kernel (nastar_capi.hip),
// included INSIDE each kernel: the kernel without a mask keeps, token for token, the body it had before the masked one existed, so its
// instruction stream is unchanged (a shared __device__ function changes how the optimiser sees the body and with it the register allocation).
// In scope: the kernel's template parameters, `a`, `rcp_sqrtW`, and `constexpr bool kMasked` / `nmask` (the neighbor_filter mask, an SGPR).
// nastar_forward_compact_heuristic_kernel shares it too: `constexpr bool kHeur` / `h0` (the caller's heuristic maps, [B, H, W]); every
// kHeur branch below is discarded in the other two kernels.  nastar_forward_compact_sources_kernel (include/nastar_sources.h) is the fourth:
// `constexpr bool kMulti` -- every non-zero cell of the start map is a source, and a parent walk ends at an unset parent only.
// nastar_forward_compact_ranked_kernel (include/nastar_levels.h) is the fifth: `constexpr bool kRanked` / `levels` -- the workgroup finds its
// map from the batch's levels (ranked_map, nastar_placement.hip.h) instead of an order array; everything behind that line is the first kernel's.
// The hand-scheduled instantiations (kAsm: the first and the fifth kernel only) decide per map whether its cost word can hold the heuristic
// instead (`stored_h`, nastar_search_asm5.hip.h); every such line sits behind `if constexpr (kAsm)` or folds away with kAsm, so the other
// kernels keep their machine code (tools/compare_device_code.py).  `constexpr bool kTicket` / `ticket_word`, `ticket_value` (the first and the
// fifth kernel only; a constexpr null elsewhere): the launch announces its own start (include/nastar_ticket.h).
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // The launch announces that it has STARTED (include/nastar_ticket.h): it was dispatched behind a barrier, so everything queued on its stream
    // before it is complete and the maps are final -- the store orders no data, hence relaxed; system scope because the command processor
    // reads the word.  Before the first return, so that a wait for this ticket is always satisfied.  The ranked kernel stores first thing.
    // The plain kernel stores BEHIND the reads of `order` / `order_bad`: a store ahead of them makes the compiler read both with vector
    // loads instead of scalar ones and hold the kernel-argument loads back behind it -- a chain of dependent memory latencies ahead of
    // the map load, 2.5 us on a launch with a lone wavefront per CU (measured: profiles/proof_ticket.json).  Without an order (the common
    // call) nothing is read in front of the store.
    if constexpr (kTicket && kRanked) {
        if (ticket_word != nullptr && blockIdx.x == 0 && threadIdx.x == 0)
            __hip_atomic_store(ticket_word, ticket_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    const int b = kRanked ? ranked_map(levels, a.B) : placed_map(a.order, a.order_bad, a.B);
    if constexpr (kTicket && !kRanked) {
        if (ticket_word != nullptr && blockIdx.x == 0 && threadIdx.x == 0)
            __hip_atomic_store(ticket_word, ticket_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        // the 18 instructions above are 72 bytes; 14 more make it 128, so that every loop behind the prologue starts where it started without
        // the ticket, modulo the 64-byte fetch line (the hand-scheduled step loops are 390 .. 480 bytes long: 8 bytes further on, some of
        // them reach into one more line per trip, which a lone wavefront per CU does not hide -- measured: profiles/proof_ticket.json)
        asm volatile("s_nop 0\n s_nop 0\n s_nop 0\n s_nop 0\n s_nop 0\n s_nop 0\n s_nop 0\n s_nop 0\n s_nop 0\n s_nop 0\n s_nop 0\n s_nop 0\n s_nop 0\n s_nop 0");
    }
    if ((unsigned)b >= (unsigned)a.B) return;  // not a permutation (and not checked: NASTAR_FLAG_CHECK_ORDER): never read or write outside the batch
    const bool lockstep = !kAsm && (a.flags & NASTAR_FLAG_LOCKSTEP);  // (forward_impl picks a compiled instantiation for it)
    if (lockstep && a.marks != nullptr && a.marks[b] == 0) return;    // not in the batch-coupled class: the early-exit launch's outputs stand
    const int lane = threadIdx.x;
    CompactDims d = a.d;
    constexpr int kCcl = kAsm ? compact_asm_ccl(LOGW) : CCL;  // cells per chunk minimum (log2): the hand-scheduled 32x32 layout keeps one per map ROW
    if constexpr (LOGH > 0 && LOGW > 0) {
        d.H = 1 << LOGH;
        d.W = 1 << LOGW;
        d.HW = 1 << (LOGH + LOGW);
        d.nchunks = d.HW >> kCcl;  // kAsm at 32x32: 32 live entries; CPL and NCp below stay 1 and 64 (entries 32..63 idle for good), as the carve expects
        d.HWp = d.HW;
        d.CPL = (d.nchunks + 63) / 64;
        d.NCp = d.CPL * 64;
        d.magicW = (uint32_t)((1ull << 32) >> LOGW) + 1u;
    }
    CompactLds l;
    if constexpr (kAsm) {  // guard rows around gc[], no dump words (nastar_search_compact.hip.h)
        l = carve_compact_asm_lds(smem, d);
        compact_store_guard_rows(l, d, lane);
    } else l = carve_compact_lds(smem, d);
    const size_t off = (size_t)b * (size_t)d.HW;

    int start_idx, goal_idx;
    constexpr int kLoadIter = (kVec4 && LOGH > 0 && LOGW > 0 && LOGH + LOGW >= 8) ? (1 << (LOGH + LOGW - 8)) : 0;
    bool any_signed = true;
    bool all_unit = false;  // kAsm: every cost is exactly 0.0 or 1.0
    // round-3 instruction stream (raw-bit keys): every cost >= +0 and 0 <= g_ratio <= 1 so that every priority is >= +0
    compact_load_map<kVec4, kLoadIter>(d, l, a.cost + off, a.start + off, a.goal + off, a.passable + off, lane, start_idx, goal_idx,
                                       kAsm ? &any_signed : nullptr, kAsm ? &all_unit : nullptr);
#ifdef NASTAR_DEV
    const bool raw = kAsm && !any_signed && !(a.flags & NASTAR_FLAG_ASM_V2) && d.gr >= 0.f && d.omg >= 0.f;
#else
    const bool raw = kAsm && !any_signed && d.gr >= 0.f && d.omg >= 0.f;
#endif
    float* hhv = nullptr;  // kHeur: fl(omg * fl(h0 + cost)) per cell, behind the compact state
    bool bad_h0 = false;
    if constexpr (kHeur) {
        hhv = reinterpret_cast<float*>(l.pdir + d.HWp);
        bad_h0 = compact_load_heuristic<kVec4>(d, l, hhv, h0 + off, lane);
    }
    const int gi = goal_idx < 0 ? 0 : goal_idx;
    const int goal_r = (int)row_magic((uint32_t)gi, d.magicW, d.W);
    const int goal_c = gi - goal_r * d.W;

    const CompactLane lc = make_compact_lane<kMasked>(d, lane, nmask);  // (kMasked: lanes 0-7 gated by the mask -- the goal-expansion test of the COUPLED note reads them too)
    int status = NASTAR_OK;
    int iters = 0;
    bool solved = false, coupled = false;
    bool goal_hit = false;
    bool stored_h = false;  // kAsm: this map keeps fl(h0 + 1.0) where its cost word was (nastar_search_asm5.hip.h); wave-uniform
    const bool probe = lockstep && a.bitmap != nullptr;
    const int budget = (lockstep && a.t_end != nullptr) ? __builtin_amdgcn_readfirstlane(*a.t_end + 1) : a.max_iters;
    uint32_t bits = 0u;  // probe: goal selections of the current 32 steps
    uint32_t* const bm = probe ? a.bitmap + (size_t)b * (size_t)a.bitmap_words : nullptr;
    if (kHeur && bad_h0) {
        status = NASTAR_ERR_BAD_HEURISTIC;  // a NaN / infinite heuristic value: this map is not searched (empty outputs)
    } else if (start_idx < 0 || goal_idx < 0) {
        status = NASTAR_ERR_UNSOLVABLE;  // not a one-hot start/goal map
    } else {
        // round-4 stream (nastar_search_asm4.hip.h) wherever raw-bit keys apply (costs >= +0, 0 <= g_ratio <= 1: every priority is >= +0); a map with a
        // negative / NaN cost takes the round-2 stream with its order-preserving key transform (nastar_search_asm.hip.h).  The development build
        // (make dev) can also select the round-3 stream and switch the 64x64 dive off: csrc/nastar_dev_flags.h, stream-equality tests.
        // half: g_ratio == 0.5 -- the two products of f = g_ratio g + (1 - g_ratio) h are exact and drop out of the key
#ifdef NASTAR_DEV
        const bool asm4 = raw && !(a.flags & NASTAR_FLAG_ASM_V3);
        const bool no_dive = (a.flags & NASTAR_FLAG_NO_DIVE) != 0;
#else
        const bool asm4 = raw;
#endif
        const bool half = asm4 && d.gr == 0.5f && d.omg == 0.5f;
        if constexpr (kMulti) compact_open_sources<kVec4, kFastDiv, kHeur>(d, l, hhv, a.start + off, lane, goal_r, goal_c, rcp_sqrtW);
        else
        if constexpr (kHeur) {  // open list = {start} (:187), g[start] = 0 (:193), keyed by the stored hh
            if (lane == 0) {
                l.gc[start_idx].x = 0.0f;
                l.cmin[start_idx >> CCL] = cmin_entry(compact_key<kFastDiv>(d, 0.0f, hhv[start_idx], rcp_sqrtW), (uint32_t)start_idx);
                l.pdir[start_idx] = (uint8_t)(PARENT_UNSET | P_PASS);
            }
            wave_sync();
        } else
        compact_open_start<kFastDiv>(d, l, lane, start_idx, goal_r, goal_c, rcp_sqrtW, raw, half, kCcl);
        int s = 0;
        if constexpr (kAsm) {
            // ONE binary tensor as cost map and obstacle map (VanillaAstar, reference astar.py:93-94): every cell the search can relax costs
            // 1.0, the cost word carries nothing and takes hh = fl(h0 + 1.0) instead -- decided here, per map, from what the load saw; no
            // flag, no status.  A start on an obstacle (cost 0, expanded all the same, :187) is opened with g = -1.0: fl(-1.0 + 1.0) = fl(0 + 0)
            // is what its first step hands on (nastar_search_unit.hip.h); its key above was formed from its cost word before that word goes.
#ifdef NASTAR_DEV
            stored_h = asm4 && !no_dive && all_unit && a.cost == a.passable;
#else
            stored_h = asm4 && all_unit && a.cost == a.passable;
#endif
            if (stored_h) {
                const bool start_blocked = l.gc[start_idx].y == 0.0f;
                compact_store_heuristic<LOGW>(l, lane, goal_r, goal_c);
                if (start_blocked && lane == 0) l.gc[start_idx].x = -1.0f;
                wave_sync();
            }
            static_assert(LOGW > 0 && LOGW == LOGH && (CPL_T == 1 || CPL_T == 4) && kFastDiv, "asm loop: 16x16, 32x32, 64x64");
            int* const log_row = kLog ? a.sel_log + (size_t)b * (size_t)a.max_iters : nullptr;
            // searching wavefronts issue ahead of the ones still loading their map or already storing their result (the launch waits for the
            // longest SEARCH): maze32 159.4 -> 157.7 us, rand32 75.6 -> 75.0 us per 4096 maps, same box, two runs each; 3-4 batches in flight unchanged at 57 M maps/s (profiles/r03/prio_*.json, prio_streams.txt)
            __builtin_amdgcn_s_setprio(3);
            constexpr bool kD = CPL_T == 4;  // only the 64x64 instantiation dives (nastar_search_asm4.hip.h)
#ifdef NASTAR_DEV
            if (asm4 && kD && no_dive) {
                if (half) s = search_loop_asm4<LOGW, kLog, false, true, false>(d.gr, d.omg, d.sqrtW, lane, goal_idx, goal_r, goal_c, a.max_iters, iters, rcp_sqrtW, log_row);
                else s = search_loop_asm4<LOGW, kLog, false, false, false>(d.gr, d.omg, d.sqrtW, lane, goal_idx, goal_r, goal_c, a.max_iters, iters, rcp_sqrtW, log_row);
            } else if (raw && !asm4 && kD && no_dive) {
                s = compact_search_loop_asm3<LOGW, kLog, false>(d, lane, goal_idx, goal_r, goal_c, a.max_iters, iters, rcp_sqrtW, log_row);
            } else if (raw && !asm4) {
                s = compact_search_loop_asm3<LOGW, kLog>(d, lane, goal_idx, goal_r, goal_c, a.max_iters, iters, rcp_sqrtW, log_row);
            } else
#endif
            if (stored_h) {
                s = half ? search_loop_asm5<LOGW, kLog, kD, true>(d.gr, d.omg, d.sqrtW, lane, goal_idx, a.max_iters, iters, rcp_sqrtW, log_row)
                         : search_loop_asm5<LOGW, kLog, kD, false>(d.gr, d.omg, d.sqrtW, lane, goal_idx, a.max_iters, iters, rcp_sqrtW, log_row);
            } else if (asm4) {
                s = half ? search_loop_asm4<LOGW, kLog, kD, true, false>(d.gr, d.omg, d.sqrtW, lane, goal_idx, goal_r, goal_c, a.max_iters, iters, rcp_sqrtW, log_row)
                         : search_loop_asm4<LOGW, kLog, kD, false, false>(d.gr, d.omg, d.sqrtW, lane, goal_idx, goal_r, goal_c, a.max_iters, iters, rcp_sqrtW, log_row);
            } else {
                s = compact_search_loop_asm<LOGW, kLog>(d, lane, goal_idx, goal_r, goal_c, a.max_iters, iters, rcp_sqrtW, log_row);
            }
            __builtin_amdgcn_s_setprio(0);
        } else
        while (iters < budget) {  // :203 for t in range(Tmax)
            uint2 mine;
            s = compact_select<CPL_T>(d, l, lane, mine);
            if (s < 0 || (s == goal_idx && !lockstep)) break;  // single exit test: open list empty (:68 would divide by zero) or goal
            if constexpr (kLog) {
                if (lane == 0) a.sel_log[(size_t)b * (size_t)a.max_iters + iters] = s;
            }
            if (probe) {
                if (s == goal_idx) bits |= 1u << (iters & 31);
                if ((iters & 31) == 31) {
                    if (lane == 0) bm[iters >> 5] = bits;
                    bits = 0u;
                }
            }
            ++iters;
            // lock-step mode: the reference's loop to the letter -- a selected goal is expanded like any cell, stays open, and the map is stepped
            // on (it may wander: NASTAR_SUMMARY_COUPLED) until the caller's step count is reached
            goal_hit |= s == goal_idx;
            if constexpr (kHeur) compact_expand<LOGW, kFastDiv, CPL_T, true>(d, l, lc, lane, s, goal_r, goal_c, rcp_sqrtW, mine, s == goal_idx, hhv);
            else
            compact_expand<LOGW, kFastDiv, CPL_T>(d, l, lc, lane, s, goal_r, goal_c, rcp_sqrtW, mine, s == goal_idx);
        }
        if (probe) {  // the words this map's search did not reach say "no goal selection"; nothing else is written
            if (lane == 0) {
                if (iters & 31) bm[iters >> 5] = bits;
                for (int w = (iters + 31) >> 5; w < a.bitmap_words; ++w) bm[w] = 0u;
            }
            return;
        }
        if (lockstep && goal_hit && lane == 0) l.gc[goal_idx].x = NASTAR_NEG_INF;  // histories holds the goal (:222-223); nothing reads its g any more
        if (kAsm ? (s != -2) : (iters < budget)) {
            if (s < 0) {
                status = NASTAR_ERR_UNSOLVABLE;
            } else {  // :219-220,:251 reached the goal: every later step of the reference is a fixed point
                if constexpr (kLog) {
                    if (lane == 0) a.sel_log[(size_t)b * (size_t)a.max_iters + iters] = s;
                }
                ++iters;
                solved = true;
                if (a.summary != nullptr || a.marks_out != nullptr) {
                    // Is this map now at a FIXED POINT of the reference's batch loop?  The reference keeps stepping a finished map until every
                    // map of the batch selects its goal in the same step (:224 the goal stays open, :251); this kernel stops here.  The two
                    // agree iff the goal's own expansion opens nothing that beats the goal: true for every g_ratio in [0.5, 1) with costs >= 0
                    // (f(n) - f(goal) = (2 g_ratio - 1) c_goal + (1 - g_ratio)(h0(n) + c_n) > 0), not for g_ratio < 0.5 with an expensive goal
                    // cell, g_ratio = 1 with a zero-cost one, or negative costs.  Detected here, reported as summary[NASTAR_SUMMARY_COUPLED].
                    const int nr = goal_r + lc.dr, nc = goal_c + lc.dc;
                    const bool inb = lc.is_nb & ((unsigned)nr < (unsigned)d.H) & ((unsigned)nc < (unsigned)d.W);
                    const int n = inb ? s + lc.off : s;
                    float2 gg = l.gc[s], gn = l.gc[n];
                    if constexpr (kAsm) {
                        if (stored_h) {  // the words read above hold hh: a cell that can be relaxed costs 1.0, a goal that is the start what the caller's map says (and its g was 0)
                            gn.y = 1.0f;
                            gg.y = 1.0f;
                            if (s == start_idx) gg = make_float2(0.0f, a.cost[off + s]);
                        }
                    }
                    const float g2 = gg.x + gg.y;
                    uint32_t kn, kg;
                    if constexpr (kHeur) {  // the stored values, for the neighbour AND the goal (h0(goal) need not be 0)
                        kn = compact_key<kFastDiv>(d, g2, hhv[n], rcp_sqrtW);
                        kg = compact_key<kFastDiv>(d, gg.x, hhv[s], rcp_sqrtW);
                    } else {
                    kn = compact_key<kFastDiv>(d, g2, d.omg * (heuristic0_fast(nr, nc, goal_r, goal_c) + gn.y), rcp_sqrtW);
                    kg = compact_key<kFastDiv>(d, gg.x, d.omg * (heuristic0_fast(goal_r, goal_c, goal_r, goal_c) + gg.y), rcp_sqrtW);
                    }
                    const bool beats = inb & (gn.x > g2) & ((kn < kg) | ((kn == kg) & (n < s)));
                    coupled = __ballot(beats) != 0ull;
                    if (coupled && a.summary != nullptr && lane == 0) a.summary[NASTAR_SUMMARY_COUPLED] = 1;
                    wave_order();
                }
                if (lane == 0) l.gc[s].x = NASTAR_NEG_INF;  // :222-223 the goal joins the closed list
            }
        }
    }
    wave_sync();
    // histories depend on the closed list only: their stores are issued first and drain under the serial backtrack
    compact_store_hist<kVec4>(d, l, lane, a.hist + off);
    if (probe) return;  // (a map without a one-hot start / goal: the early-exit launch reported it, it is never marked)
    if (lane == 0) {
        a.iters[b] = iters;
        a.status[b] = status;
        if (a.marks_out != nullptr) a.marks_out[b] = coupled ? 1 : 0;
        if (status != NASTAR_OK && a.summary) a.summary[status] = 1;  // plain idempotent store: the word may be host-mapped (no atomics over PCIe)
        if (a.order_out) note_completion(a.order_out, a.B, b);
        // (the COUPLED note above is a summary cell like any other: it must be visible before this search counts itself -- ADVICE r5)
        if (a.done_counter) note_done(a.done_counter, a.summary, a.B, status != NASTAR_OK || coupled);
    }
    if (goal_idx >= 0 && !(kHeur && bad_h0)) compact_backtrack<(LOGW == LOGH ? LOGW : 0)>(d, l, lane, kMulti ? -1 : start_idx, goal_idx, solved ? d.HW : iters - 1);
    compact_store_outputs<kVec4, false>(d, l, lane, a.hist + off, a.paths + off,
                                        a.packed ? a.packed + (size_t)b * (size_t)(d.HW >> 2) : nullptr);
    const RouteOut ro = kernel_route_args<offsetof(FwdCArgs, route)>();  // (a.route, read here: nastar_routes.hip.h)
    if (ro.routes != nullptr) {  // wave-uniform; null unless the launch came through include/nastar_routes.h
        // (a stored_h map has no cost word: every cell the search opened is passable and costs 1, the start's cost is read from the caller's map)
        const float start_cost = (kAsm && stored_h) ? a.cost[off + start_idx] : 0.f;
        const int n = route_walk(l.pdir, lane, kMulti ? -1 : start_idx, goal_idx, solved ? d.HW : iters - 1, goal_idx >= 0 && !(kHeur && bad_h0),
                                 [&](int c, uint32_t code) { return compact_parent_of(d, c, code); },
                                 [&](int c) { return (kAsm && stored_h) ? (c == start_idx ? start_cost : 1.0f) : l.gc[c].y; }, ro, b);
        route_fill_tail(ro, b, n, lane);
    }
