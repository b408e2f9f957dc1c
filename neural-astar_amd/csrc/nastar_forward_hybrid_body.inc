// nastar_forward_hybrid_body.inc -- the body of nastar_forward_hybrid_kernel and nastar_forward_hybrid_masked_kernel (nastar_search_hybrid.hip.h),
// included INSIDE each kernel so that the kernel without a mask keeps its instruction stream (see nastar_forward_compact_body.inc).
// In scope: kFastDiv, kLock, `a`, and `constexpr bool kMasked` / `nmask` (the neighbor_filter mask, an SGPR).
// nastar_forward_hybrid_heuristic_kernel shares it too: `constexpr bool kHeur` / `h0` (the caller's heuristic maps, [B, H, W], read cell by
// cell next to the cost in the step's one HBM round trip); every kHeur branch is discarded in the other two kernels.
// nastar_forward_hybrid_sources_kernel (include/nastar_sources.h) is the fourth: `constexpr bool kMulti` -- the searching wavefront opens
// every non-zero cell of the start map in a pass before its first step, and a parent walk ends at an unset parent only.
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int b = blockIdx.x;
    if constexpr (kLock) {
        if (a.marks != nullptr && a.marks[b] == 0) return;  // not in the batch-coupled class: the early-exit launch's outputs stand
    }
    const int lane = threadIdx.x;
    const HybridDims d = a.d;
    const int HWp = d.nchunks * 64;
    unsigned long long* const cmin = reinterpret_cast<unsigned long long*>(smem);
    unsigned long long* const smin = cmin + d.nsuper * 64;
    unsigned char* const slab = a.workspace + (size_t)b * a.slab_bytes;
    float* const g = reinterpret_cast<float*>(slab);
    uint8_t* const pdir = reinterpret_cast<uint8_t*>(g + HWp);
    const int* const hdr = reinterpret_cast<const int*>(slab + hybrid_header_offset(d.HW));
    const size_t off = (size_t)b * (size_t)d.HW;
    const float* cost = a.cost + off;
    const float* const h0m = kHeur ? h0 + off : nullptr;
    const bool probe = kLock && a.bitmap != nullptr;
    const int budget = (kLock && a.t_end != nullptr) ? __builtin_amdgcn_readfirstlane(*a.t_end + 1) : a.max_iters;

    // ---- start / goal from the fill launch; empty open list -------------------------------------------------------------
    const int sidx = __builtin_amdgcn_readfirstlane(hdr[0]), gidx = __builtin_amdgcn_readfirstlane(hdr[1]);
    for (int c = lane; c < d.nsuper * 64; c += 64) cmin[c] = ~0ull;
    for (int c = lane; c < d.spl * 64; c += 64) smin[c] = ~0ull;
    const int gi = gidx < 0 ? 0 : gidx;
    int goal_c;
    const int goal_r = hybrid_row(gi, d, goal_c);
    __syncthreads();
    float h_start = 0.f;  // :191-192 h = h0 + cost at the start cell (wave-uniform)
    if (sidx >= 0) {
        int sc;
        const int sr = hybrid_row(sidx, d, sc);
        if constexpr (kHeur) h_start = h0m[sidx] + cost[sidx];
        else
        h_start = heuristic0(sr, sc, goal_r, goal_c) + cost[sidx];
    }
    unsigned long long first_sel = ~0ull;  // kMulti: (key << 32 | cell) of the first selection
    if constexpr (kMulti) {
        if (sidx >= 0 && gidx >= 0) first_sel = hybrid_open_sources<kFastDiv, kHeur>(d, g, pdir, cmin, smin, cost, h0m, a.start + off, lane, goal_r, goal_c);
    } else
    if (lane == 0 && sidx >= 0) {  // open list = {start} (:187), g[start] = 0 (:193); the start is expanded even on an obstacle
        const uint32_t k0 = hybrid_key<kFastDiv>(d, 0.0f, h_start);
        const unsigned long long e = ((unsigned long long)k0 << 32) | (uint32_t)sidx;
        g[sidx] = 0.0f;
        pdir[sidx] = (uint8_t)(PARENT_UNSET | P_PASS);
        cmin[sidx >> 6] = e;
        smin[sidx >> 12] = e;
    }
    __syncthreads();

    int dr, dc;
    neighbour_delta(lane & 7, dr, dc);
    const bool nb_on = kMasked && neighbour_enabled(lane, nmask);  // masked kernel: lanes 0-7 that the neighbor_filter opens (loop invariant)
    int status = NASTAR_OK;
    int iters = 0;
    bool solved = false, goal_hit = false, coupled = false;
    uint32_t bits = 0u;  // probe: goal selections of the current 32 steps
    uint32_t* const bm = probe ? a.bitmap + (size_t)b * (size_t)a.bitmap_words : nullptr;
    if (kHeur && __builtin_amdgcn_readfirstlane(hdr[2]) != 0) {
        status = NASTAR_ERR_BAD_HEURISTIC;  // the fill launch met a NaN / infinite heuristic value: this map is not searched
    } else if (sidx < 0 || gidx < 0) {
        status = NASTAR_ERR_UNSOLVABLE;  // not a one-hot start / goal map
    } else {
        // (key << 32 | cell) of the next selection, wave-uniform in scalar registers; ~0 = open list empty
        uint32_t sel_key = hybrid_key<kFastDiv>(d, 0.0f, __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(h_start))));
        uint32_t sel_cell = (uint32_t)sidx;
        if constexpr (kMulti) {
            sel_key = (uint32_t)(first_sel >> 32);
            sel_cell = (uint32_t)first_sel;
        }
        while (iters < budget) {  // :203
            // ---- select: the entry the previous step left behind names s* (no LDS read, no reduction on this path) -------------
            const int s = (int)sel_cell;
            if (s < 0) {  // every entry idle (~0ull: key KEY_INF, cell ~0): open list empty (:68 would divide by zero)
                status = NASTAR_ERR_UNSOLVABLE;
                break;
            }
            if (a.sel_log != nullptr && !probe && lane == 0) a.sel_log[(size_t)b * (size_t)a.max_iters + iters] = s;
            const bool at_goal = s == gidx;
            if constexpr (kLock) {
                if (probe) {
                    if (at_goal) bits |= 1u << (iters & 31);
                    if ((iters & 31) == 31) {
                        if (lane == 0) bm[iters >> 5] = bits;
                        bits = 0u;
                    }
                }
            }
            ++iters;
            if (!kLock && at_goal) {
                // :219-220,:251 every later step of the reference is a fixed point -- unless the goal's own expansion would open a cell that beats
                // it (nastar_capi.hip, same test): reported as summary[NASTAR_SUMMARY_COUPLED] and, per map, in marks[]
                if (a.summary != nullptr || a.marks_out != nullptr) {
                    if constexpr (kHeur) coupled = hybrid_goal_beaten_heuristic<kFastDiv>(d, g, cost, h0m, s, nb_on, dr, dc);
                    else
                    if constexpr (kMasked) coupled = hybrid_goal_beaten_gated<kFastDiv>(d, g, cost, s, nb_on, dr, dc, goal_r, goal_c);
                    else coupled = hybrid_goal_beaten<kFastDiv>(d, g, cost, s, lane, dr, dc, goal_r, goal_c);
                }
                if (lane == 0) g[s] = NASTAR_NEG_INF;  // :222-223 the goal joins the closed list
                solved = true;
                break;
            }
            goal_hit |= at_goal;
            const int C = s >> 6, S = s >> 12;
            // ---- the open list WITHOUT the chunk / super-chunk of s*, as the previous step left it (LDS, issued ahead of the HBM loads) ----
            const unsigned long long ev = cmin[S * 64 + lane];
            unsigned long long e0 = (lane * d.spl == S) ? ~0ull : smin[lane * d.spl];
            for (int j = 1; j < d.spl; ++j) {  // (maps above 512x512: several super-chunk entries per lane, contiguous -- the first minimal one wins)
                const unsigned long long ej = (lane * d.spl + j == S) ? ~0ull : smin[lane * d.spl + j];
                e0 = (uint32_t)(ej >> 32) < (uint32_t)(e0 >> 32) ? ej : e0;
            }
            int c;
            const int r = hybrid_row_nb(s, d, c);
            const int nr = r + dr, nc = c + dc;
            const bool inb = (kMasked ? nb_on : (lane < 8)) & ((unsigned)nr < (unsigned)d.H) & ((unsigned)nc < (unsigned)d.W);  // conv2d zero padding
            const int n = inb ? s + dr * d.W + dc : s;
            const int ic = C * 64 + lane;
            const bool icv = ic < d.HW;
            global_step_fence();  // the previous step's g / pdir stores have reached L2
            // ---- ONE round trip: everything this step reads from HBM --------------------------------------------------
            const float gs = g[s];
            const float gn = g[n];
            const float gc = g[ic];
            const float cs = cost[s];
            const float cn = cost[n];
            const float cc = cost[icv ? ic : 0];
            float hn, hc;
            if constexpr (kHeur) {
                hn = h0m[n];
                hc = h0m[icv ? ic : 0];
            }
            // ---- in the shadow of that round trip: nothing below needs a loaded value until `g2` -------------------------
            // rest of the super-chunk of s* (its 64 chunk entries but the one of s*) and rest of the map (every other super-chunk): entries
            // ascend with the lane, so the first lane that holds the minimal key holds the first minimal entry
            const uint32_t kS = lane == (C & 63) ? KEY_INF : (uint32_t)(ev >> 32);
            const uint32_t kE = (uint32_t)(e0 >> 32);
            uint32_t mS, mE;
            wave_min_scalar_u32x2(kS, kE, mS, mE);
            const uint32_t cS = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)ev, __builtin_ctzll(__ballot(kS == mS)));
            const uint32_t cE = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)e0, __builtin_ctzll(__ballot(kE == mE)));
            if constexpr (!kHeur) {
            int icc;
            const int icr = hybrid_row_nb(icv ? ic : 0, d, icc);
            hn = heuristic0(nr, nc, goal_r, goal_c);
            hc = heuristic0(icr, icc, goal_r, goal_c);
            // (the compiler otherwise sinks both heuristics below the first use of a loaded value, into regions predicated on `upd` / `open_c`:
            //  a lone wavefront pays for predicated-off lanes anyway, and there they sit behind the round trip instead of inside it)
            asm volatile("" : "+v"(hn), "+v"(hc) : : "memory");
            }
            // ---- the loaded values ------------------------------------------------------------------------------------------
            const float g2 = gs + cs;                                              // :234 step cost of the node being LEFT
            const bool upd = inb & (gn > g2);                                      // :229,:235
            // chunk minimum without s* (lock-step: a selected goal stays on the open list, :224): open <=> finite g
            const bool open_c = icv & (fabsf(gc) < NASTAR_POS_INF) & ((ic != s) | (kLock && at_goal));
            uint32_t kn_all = hybrid_key<kFastDiv>(d, g2, hn + cn);
            uint32_t kc_all = hybrid_key<kFastDiv>(d, gc, hc + cc);                // (of +-inf for cells that are not open: discarded)
            asm volatile("" : "+v"(kn_all), "+v"(kc_all));                         // both keys for all lanes, side by side (no predicated regions)
            const uint32_t kn = upd ? kn_all : KEY_INF;
            const uint32_t kc = open_c ? kc_all : KEY_INF;
            // the chunk of s* without s* (64 lanes, ascending cells) and, beside it, the relaxed neighbours (lanes 0..7 in raster order: ascending cells)
            uint32_t mC, mN;
            wave_min_scalar_u32_and8(kc, kn, mC, mN);
            const uint32_t cC = (uint32_t)(C * 64 + __builtin_ctzll(__ballot(kc == mC)));   // (mC == KEY_INF: every lane matches, masked below)
            const uint32_t cN = (uint32_t)__builtin_amdgcn_readlane(n, __builtin_ctzll(__ballot(kn == mN)));
            // ---- stores: closed list, relaxed neighbours (:222-225, :238-249) ----------------------------------------
            if (lane == 0 && !(kLock && at_goal)) g[s] = NASTAR_NEG_INF;
            if (upd) {
                g[n] = g2;
                pdir[n] = (uint8_t)(P_PASS | (uint32_t)lane);
            }
            // ---- open list (LDS executes a wavefront's operations in order; nothing is read back in this step) ------------
            // chunk of s*: its cells without s* ...; super-chunk of s*: its other chunks and that; the neighbours enter both levels by ds_min
            const uint32_t kCS = min(mC, mS);
            const uint32_t cCS = min(mC == kCS ? cC : 0xFFFFFFFFu, mS == kCS ? cS : 0xFFFFFFFFu);
            const unsigned long long en = ((unsigned long long)kn << 32) | (uint32_t)n;
            if (lane == 0) {
                cmin[C] = mC == KEY_INF ? ~0ull : (((unsigned long long)mC << 32) | cC);
                smin[S] = kCS == KEY_INF ? ~0ull : (((unsigned long long)kCS << 32) | cCS);
            }
            wave_order();
            if (upd) {
                atomicMin(&cmin[n >> 6], en);                                      // :242 (re)opened neighbours enter their chunk's minimum
                atomicMin(&smin[n >> 12], en);                                     // ... and their super-chunk's (a neighbour may sit in another one)
            }
            wave_order();
            // ---- the next selection: first-index minimum of {rest of the map, super-chunk of s* without s*, relaxed neighbours} ----
            const uint32_t kX = min(mE, mN);
            const uint32_t cX = min(mE == kX ? cE : 0xFFFFFFFFu, mN == kX ? cN : 0xFFFFFFFFu);
            sel_key = min(kCS, kX);
            sel_cell = min(kCS == sel_key ? cCS : 0xFFFFFFFFu, kX == sel_key ? cX : 0xFFFFFFFFu);
            if (sel_key == KEY_INF) sel_cell = 0xFFFFFFFFu;
        }
    }
    global_step_fence();
    if constexpr (kLock) {
        if (probe) {  // the words this map's search did not reach say "no goal selection"
            if (lane == 0) {
                if (iters & 31) bm[iters >> 5] = bits;
                for (int w = (iters + 31) >> 5; w < a.bitmap_words; ++w) bm[w] = 0u;
            }
            return;
        }
        if (goal_hit && lane == 0) g[gidx] = NASTAR_NEG_INF;  // histories holds the goal (:222-223); nothing reads its g any more
    }
    if (lane == 0) {
        a.iters[b] = iters;
        a.status[b] = status;
        if (a.marks_out != nullptr) a.marks_out[b] = coupled ? 1 : 0;
        if (a.summary) {
            if (status != NASTAR_OK) a.summary[status] = 1;
            if (coupled) a.summary[NASTAR_SUMMARY_COUPLED] = 1;
        }
    }

    // ---- backtrack (:96-125): walk to the start, cap = this map's own step count in the budget-truncated case ----------
    if (gidx >= 0 && lane == 0 && !(kHeur && status == NASTAR_ERR_BAD_HEURISTIC)) {
        const int cap = solved ? d.HW : iters - 1;
        uint32_t m = pdir[gidx];
        pdir[gidx] = (uint8_t)(m | P_PATH);
        uint32_t code = m & P_DIRMASK;
        if (code != PARENT_UNSET) {
            int pdr, pdc;
            neighbour_delta((int)code, pdr, pdc);
            int loc = gidx - (pdr * d.W + pdc);
            for (int k2 = 0; k2 < cap; ++k2) {
                const uint32_t ml = pdir[loc];
                pdir[loc] = (uint8_t)(ml | P_PATH);
                if (!kMulti && loc == sidx) break;
                const uint32_t cd = ml & P_DIRMASK;
                if (cd == PARENT_UNSET) break;
                neighbour_delta((int)cd, pdr, pdc);
                loc -= pdr * d.W + pdc;
            }
        }
    }
    global_step_fence();
    const RouteOut ro = kernel_route_args<offsetof(FwdHybridArgs, route)>();  // (a.route, read here: nastar_routes.hip.h)
    if (ro.routes != nullptr) {  // wave-uniform; parents from the slab, costs from the caller's tensor; the -1 tail: store launch
        route_walk(pdir, lane, kMulti ? -1 : sidx, gidx, solved ? d.HW : iters - 1, gidx >= 0 && !(kHeur && status == NASTAR_ERR_BAD_HEURISTIC),
                   [&](int c, uint32_t code) {
                       int pdr, pdc;
                       neighbour_delta((int)code, pdr, pdc);
                       return c - (pdr * d.W + pdc);
                   },
                   [&](int c) { return cost[c]; }, ro, b);
    }
