// nastar_search_kernels.hip.h -- the device code of the search translation unit (nastar_capi.hip): the argument struct of the LDS-resident
// search kernels, their placement / completion helpers, the kernels that wrap nastar_forward_compact_body.inc, the unit-cost kernel, and the
// small kernels around a search (order check, heuristic, pack / unpack, the batch loop's stopping step).  Host code -- argument checks and
// kernel choice -- stays in nastar_capi.hip, which includes this file behind the search headers (and, in the development build, behind
// nastar_dev_flags.h).
#pragma once
#include "nastar_search_compact.hip.h"
#include "nastar_search_unit.hip.h"
#include "nastar_routes.hip.h"

namespace nastar {

// ---- forward, compact LDS state (nastar_search_compact.hip.h): the default for every map that fits LDS ------------------
struct FwdCArgs {
    const float* cost;
    const float* start;
    const float* goal;
    const float* passable;
    float* hist;
    long long* paths;
    int* sel_log;
    int* iters;
    int* status;
    uint8_t* packed;
    const int* order;  // optional placement: workgroup i runs map order[i] (a permutation of 0..B-1), nullptr = identity
    int* order_out;    // optional [B + 1]: the maps in REVERSE order of search completion (the placement for the next visit); [B] = counter
    int* summary;      // optional [NASTAR_SUMMARY_WORDS]: summary[c] = 1 when some map of this launch ends with per-map status c != 0 (device or host-mapped)
    const int* order_bad;  // optional: *order_bad != 0 (written by nastar_order_check_kernel earlier on the stream) = `order` is not a permutation, ignore it
    int* done_counter;     // optional device cell (0 on entry, 0 again at the end): the workgroup whose search finishes LAST sets summary[0] = 1
    int* marks_out;        // early-exit launch, optional [B] (NASTAR_FLAG_MARK_COUPLED): 1 = this map reached its goal but is not at a fixed point of the reference's batch loop
    const int* marks;      // lock-step launches, optional [B]: search only the maps marked 1 (the others return at once: their outputs stand)
    const int* t_end;      // lock-step FINAL launch, optional device cell: the budget is *t_end + 1 steps
    uint32_t* bitmap;      // lock-step PROBE launch: [B][bitmap_words], bit t = the goal was selected at step t; no outputs are written
    int bitmap_words;
    int max_iters;
    int B;
    int flags;
    CompactDims d;
    RouteOut route;        // optional (include/nastar_routes.h): the ordered route of every map, its length and cost; null for every entry point of nastar.h
};

// which map this workgroup searches: `order[blockIdx.x]`, unless the launch was asked to check `order` (NASTAR_FLAG_CHECK_ORDER) and the
// check kernel, earlier on the same stream, found that it is not a permutation of 0..B-1 -- then the natural order (every map is searched)
__device__ __forceinline__ int placed_map(const int* order, const int* order_bad, int B)
{
    if (order == nullptr || (order_bad != nullptr && *order_bad != 0)) return (int)blockIdx.x;
    return order[blockIdx.x];
}

// order_out: this search's rank by completion time, counted from the end -- the longest searches come first next time.  The counter cell
// order_out[B] wraps at B (atomicInc): B completions bring it back to where it started (0 for a zeroed buffer) and every rank in [0, B) is
// handed out exactly once WHATEVER the cell held on entry -- a buffer that was not zeroed gets a rotated, still complete order.
__device__ __forceinline__ void note_completion(int* order_out, int B, int b)
{
    unsigned pos = atomicInc(reinterpret_cast<unsigned*>(order_out + B), (unsigned)B - 1u);
    if (pos >= (unsigned)B) pos = (unsigned)B - 1u;  // a cell that held garbage >= B: only the first increment sees it, and rank B-1 is the one nobody else gets
    order_out[B - 1 - (int)pos] = b;
}

// completion_counter of nastar_forward_ex: every search counts itself when it ENDS (before its backtrack and output stores); the last one
// publishes summary[0] = 1.  A workgroup that wrote a summary cell makes it visible system-wide BEFORE it counts (release), the last one
// orders its flag store behind the count it observed (acquire): a host that sees summary[0] != 0 in pinned memory sees every cell of the launch.
__device__ __forceinline__ void note_done(int* counter, int* summary, int B, bool wrote_summary)
{
    if (wrote_summary) __threadfence_system();
    const unsigned pos = atomicInc(reinterpret_cast<unsigned*>(counter), (unsigned)B - 1u);
    if (pos == (unsigned)B - 1u && summary) {
        __threadfence_system();
        __hip_atomic_store(summary, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// NASTAR_FLAG_CHECK_ORDER: is `order` a permutation of 0..B-1?  ONE workgroup, a bitmap of B bits in LDS; writes *bad = 0 / 1 (always)
// and, when it is not, summary[NASTAR_SUMMARY_BAD_ORDER] = 1.  The search / replay kernels that follow on the stream read *bad.
__global__ __launch_bounds__(1024) void nastar_order_check_kernel(const int* __restrict__ order, int B, int* __restrict__ bad, int* summary)
{
    extern __shared__ unsigned bitmap[];
    __shared__ int any_bad;
    const int tid = threadIdx.x, nw = (B + 31) >> 5;
    if (tid == 0) any_bad = 0;
    for (int i = tid; i < nw; i += 1024) bitmap[i] = 0u;
    __syncthreads();
    bool mine = false;
    for (int i = tid; i < B; i += 1024) {
        const int v = order[i];
        if ((unsigned)v >= (unsigned)B) mine = true;
        else if (atomicOr(&bitmap[v >> 5], 1u << (v & 31)) & (1u << (v & 31))) mine = true;  // named twice: some other map is never named
    }
    if (mine) any_bad = 1;
    __syncthreads();
    if (tid == 0) {
        *bad = any_bad;
        if (any_bad && summary) summary[NASTAR_SUMMARY_BAD_ORDER] = 1;
    }
}

// LOGH > 0 && LOGW > 0: the map is exactly (1<<LOGH) x (1<<LOGW) (compile-time sizes, immediate ds offsets).
// CPL_T: chunk minima per lane (1 or 4) when known at compile time, 0 = runtime.
// kAsm: the selection/expansion loop is a hand-scheduled instruction stream (nastar_search_asm4 / _asm3 / _asm.hip.h; 16x16, 32x32, 64x64)
// kMasked: the neighbourhood is DifferentiableAstar.neighbor_filter (nmask, see neighbour_enabled) instead of the Moore-8 stencil; compiled
// step loops only (kAsm = false).  Both kernels share one body, nastar_forward_compact_body.inc.
// ticket_word / ticket_value (this kernel and the ranked one only: `constexpr bool kTicket`): the launch announces its own START -- workgroup 0
// stores the value to the word before anything else (include/nastar_ticket.h: what the proof's side stream waits for instead of an event
// in front of this launch).  Null for every entry point but nastar_forward_proved.  Kernel arguments of their own behind rcp_sqrtW, for the
// reason given at `levels` below.
template <bool kVec4, int LOGW, int LOGH, int CPL_T, bool kFastDiv, bool kLog, bool kAsm = false>
__global__ __launch_bounds__(64) void nastar_forward_compact_kernel(const FwdCArgs a, const float rcp_sqrtW, unsigned long long* __restrict__ ticket_word,
                                                                    const unsigned long long ticket_value)
{
    constexpr bool kMasked = false, kHeur = false, kMulti = false, kRanked = false, kTicket = true;
    constexpr uint32_t nmask = NASTAR_NEIGHBORS_MOORE8;
    constexpr const float* h0 = nullptr;
    constexpr const int* levels = nullptr;
#include "nastar_forward_compact_body.inc"
}

// the first kernel with its placement computed IN the launch (include/nastar_levels.h: nastar_forward_levels): workgroup i searches
// ranked_map(levels, B) (nastar_placement.hip.h) -- no sort launch in front, no order array.  Instantiated for the hand-scheduled streams only.
// `levels` is a kernel argument of its own, behind rcp_sqrtW: a member appended to FwdCArgs would move rcp_sqrtW (and nmask, h0) in the
// argument segment of EVERY kernel that takes the struct, and with it their scalar-load offsets.
template <bool kVec4, int LOGW, int LOGH, int CPL_T, bool kFastDiv, bool kLog, bool kAsm>
__global__ __launch_bounds__(64) void nastar_forward_compact_ranked_kernel(const FwdCArgs a, const float rcp_sqrtW, const int* __restrict__ levels,
                                                                           unsigned long long* __restrict__ ticket_word, const unsigned long long ticket_value)
{
    constexpr bool kMasked = false, kHeur = false, kMulti = false, kRanked = true, kTicket = true;
    constexpr uint32_t nmask = NASTAR_NEIGHBORS_MOORE8;
    constexpr const float* h0 = nullptr;
#include "nastar_forward_compact_body.inc"
}

// the compiled step loop with the neighbourhood of a neighbor_filter (nastar_forward_ex_masked): nmask is a kernel argument (an SGPR)
template <bool kVec4, int LOGW, int LOGH, int CPL_T, bool kFastDiv, bool kLog>
__global__ __launch_bounds__(64) void nastar_forward_compact_masked_kernel(const FwdCArgs a, const float rcp_sqrtW, const uint32_t nmask)
{
    constexpr bool kAsm = false, kMasked = true, kHeur = false, kMulti = false, kRanked = false, kTicket = false;
    constexpr unsigned long long* ticket_word = nullptr;
    constexpr unsigned long long ticket_value = 0;
    constexpr const float* h0 = nullptr;
    constexpr const int* levels = nullptr;
#include "nastar_forward_compact_body.inc"
}

// the compiled step loop with a caller-supplied heuristic (nastar_forward_ex_heuristic): h0 = the heuristic maps [B, H, W].  Load time
// stores hh = fl((1-g_ratio) fl(h0 + cost)) per cell in a third LDS array (13 B per cell, compact_heur_lds_bytes); the step reads it
// beside (g, cost) and computes no heuristic.  It always takes the neighbourhood mask (NASTAR_NEIGHBORS_MOORE8 for the default filter).
template <bool kVec4, int LOGW, int LOGH, int CPL_T, bool kFastDiv, bool kLog>
__global__ __launch_bounds__(64) void nastar_forward_compact_heuristic_kernel(const FwdCArgs a, const float rcp_sqrtW, const uint32_t nmask,
                                                                              const float* __restrict__ h0)
{
    constexpr bool kAsm = false, kMasked = true, kHeur = true, kMulti = false, kRanked = false, kTicket = false;
    constexpr unsigned long long* ticket_word = nullptr;
    constexpr unsigned long long ticket_value = 0;
    constexpr const int* levels = nullptr;
#include "nastar_forward_compact_body.inc"
}

// the compiled step loop of a MULTI-SOURCE search (include/nastar_sources.h: nastar_forward_sources): every non-zero cell of the start map is
// open with g = 0 when the search begins (compact_open_sources), and a parent walk ends at an unset parent.  Two families: kHeur = false, the
// masked kernel's step with the built-in heuristic (h0 is not read); kHeur = true, the heuristic kernel's.  Both take the neighbourhood mask.
template <bool kVec4, int LOGW, int LOGH, int CPL_T, bool kFastDiv, bool kLog, bool kHeur>
__global__ __launch_bounds__(64) void nastar_forward_compact_sources_kernel(const FwdCArgs a, const float rcp_sqrtW, const uint32_t nmask,
                                                                            const float* __restrict__ h0)
{
    constexpr bool kAsm = false, kMasked = true, kMulti = true, kRanked = false, kTicket = false;
    constexpr unsigned long long* ticket_word = nullptr;
    constexpr unsigned long long ticket_value = 0;
    constexpr const int* levels = nullptr;
#include "nastar_forward_compact_body.inc"
}

// ---- forward, UNIT-COST layout (nastar_search_unit.hip.h; NASTAR_FLAG_UNIT_COST): cost map == obstacle map, every value 0.0 or 1.0 ----
// 5.5 B/cell: 29 maps of 32x32 per CU instead of 16 -- with several batches in flight throughput follows the resident maps per CU.
template <int LOGW, bool kDive>
__global__ __launch_bounds__(64) void nastar_forward_unit_kernel(const FwdCArgs a, const float rcp_sqrtW)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int W = 1 << LOGW, HW = W * W;
    const int b = placed_map(a.order, a.order_bad, a.B);
    if ((unsigned)b >= (unsigned)a.B) return;  // not a permutation (and not checked: NASTAR_FLAG_CHECK_ORDER): never read or write outside the batch
    const int lane = threadIdx.x;
    const CompactDims& d = a.d;
    const UnitLds l = carve_unit_lds<LOGW>(smem);
    const size_t off = (size_t)b * (size_t)HW;
    int start_idx, goal_idx;
    bool bad;
    unit_load_map<LOGW>(l, a.cost + off, a.start + off, a.goal + off, lane, start_idx, goal_idx, bad);
    const int gi = goal_idx < 0 ? 0 : goal_idx;
    const int goal_r = gi >> LOGW, goal_c = gi & (W - 1);
    int status = NASTAR_OK;
    int iters = 0;
    bool solved = false;
    if (bad) {
        status = NASTAR_ERR_NOT_UNIT_COST;  // the caller's promise does not hold for this map: empty outputs, never a wrong search
    } else if (start_idx < 0 || goal_idx < 0) {
        status = NASTAR_ERR_UNSOLVABLE;  // not a one-hot start/goal map
    } else {
        const bool half = d.gr == 0.5f && d.omg == 0.5f;
        if (half) unit_open_start<LOGW, true>(d, l, lane, start_idx, goal_r, goal_c, rcp_sqrtW);
        else unit_open_start<LOGW, false>(d, l, lane, start_idx, goal_r, goal_c, rcp_sqrtW);
        __builtin_amdgcn_s_setprio(3);
        int s;
        if (half) s = search_loop_asm4<LOGW, false, kDive, true, true>(d.gr, d.omg, d.sqrtW, lane, goal_idx, goal_r, goal_c, a.max_iters, iters, rcp_sqrtW, nullptr);
        else s = search_loop_asm4<LOGW, false, kDive, false, true>(d.gr, d.omg, d.sqrtW, lane, goal_idx, goal_r, goal_c, a.max_iters, iters, rcp_sqrtW, nullptr);
        __builtin_amdgcn_s_setprio(0);
        if (s != -2) {
            if (s < 0) {
                status = NASTAR_ERR_UNSOLVABLE;
            } else {  // :219-220,:251 reached the goal: every later step of the reference is a fixed point
                ++iters;
                solved = true;
                if (lane == 0) l.g[s] = NASTAR_NEG_INF;  // :222-223 the goal joins the closed list
            }
        }
    }
    wave_sync();
    unit_store_hist<LOGW>(l, lane, a.hist + off, bad);
    if (lane == 0) {
        a.iters[b] = iters;
        a.status[b] = status;
        if (status != NASTAR_OK && a.summary) a.summary[status] = 1;  // plain idempotent store: the word may be host-mapped (no atomics over PCIe)
        if (a.order_out) note_completion(a.order_out, a.B, b);
        if (a.done_counter) note_done(a.done_counter, a.summary, a.B, status != NASTAR_OK);
    }
    if (goal_idx >= 0 && !bad) {
        CompactLds cl;  // the backtrack reads and marks parents only
        cl.gc = nullptr; cl.cmin = l.cmin; cl.dump = nullptr; cl.pdir = l.pdir;
        compact_backtrack<LOGW>(d, cl, lane, start_idx, goal_idx, solved ? HW : iters - 1);
    }
    unit_store_paths<LOGW>(l, lane, a.paths + off, a.packed ? a.packed + (size_t)b * (size_t)(HW >> 2) : nullptr, bad);
    const RouteOut ro = kernel_route_args<offsetof(FwdCArgs, route)>();  // (a.route, read here: nastar_routes.hip.h)
    if (ro.routes != nullptr) {  // no cost word in LDS: every cell the search opened is passable and costs 1, the start's cost is read
        const float start_cost = start_idx >= 0 ? a.cost[off + start_idx] : 0.f;
        const int n = route_walk(l.pdir, lane, start_idx, goal_idx, solved ? HW : iters - 1, goal_idx >= 0 && !bad,
                                 [&](int c, uint32_t code) { return compact_parent_of(d, c, code); },
                                 [&](int c) { return c == start_idx ? start_cost : 1.0f; }, ro, b);
        route_fill_tail(ro, b, n, lane);
    }
}



// ---- get_heuristic standalone (parity/debug) ------------------------------------------------------------
__global__ __launch_bounds__(64) void nastar_heuristic_kernel(const float* goal, float* out, int H, int W, uint32_t magicW)
{
    const int b = blockIdx.x, lane = threadIdx.x, HW = H * W;
    const float* gm = goal + (size_t)b * HW;
    int gidx = -1;
    for (int i = lane; i < HW; i += 64)
        if (gm[i] != 0.f) gidx = i;
    gidx = wave_max_i32(gidx);
    if (gidx < 0) gidx = 0;
    const int gr = (int)row_magic((uint32_t)gidx, magicW, W), gc = gidx - gr * W;
    for (int i = lane; i < HW; i += 64) {
        int r = (int)row_magic((uint32_t)i, magicW, W), c = i - r * W;
        out[(size_t)b * HW + i] = heuristic0(r, c, gr, gc);
    }
}

// ... for maps above 65,535 cells (the large-map kernel's sizes): rows by integer division, the goal cell found by all lanes of a workgroup per map
__global__ __launch_bounds__(256) void nastar_heuristic_large_kernel(const float* goal, float* out, int H, int W)
{
    __shared__ int s_goal;
    const int b = blockIdx.x, HW = H * W;
    const float* gm = goal + (size_t)b * HW;
    if (threadIdx.x == 0) s_goal = 0;
    __syncthreads();
    int gidx = -1;
    for (int i = threadIdx.x; i < HW; i += 256)
        if (gm[i] != 0.f) gidx = i;
    if (gidx >= 0) atomicMax(&s_goal, gidx);
    __syncthreads();
    const int gr = s_goal / W, gc = s_goal - gr * W;
    for (int i = threadIdx.x; i < HW; i += 256) {
        const int r = i / W, c = i - r * W;
        out[(size_t)b * HW + i] = heuristic0(r, c, gr, gc);
    }
}

// ---- AstarOutput <-> bit-packed masks (what the multi-GPU all-gather moves: 2 bits per cell instead of 12 bytes) ----
// packed row layout: [ceil(HW/8) bytes of histories bits | ceil(HW/8) bytes of path bits], MSB = first cell (numpy.packbits)
__global__ __launch_bounds__(256) void nastar_pack_kernel(const float* __restrict__ hist, const long long* __restrict__ paths,
                                                          uint8_t* __restrict__ packed, int B, int HW, int nb)
{
    const long long total = (long long)B * nb;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(t / nb), j = (int)(t - (long long)b * nb);
        const size_t base = (size_t)b * HW + (size_t)j * 8;
        uint32_t hb = 0, pb = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (j * 8 + k < HW) {
                hb |= (hist[base + k] != 0.f ? 1u : 0u) << (7 - k);
                pb |= (paths[base + k] != 0 ? 1u : 0u) << (7 - k);
            }
        }
        packed[(size_t)b * 2 * nb + j] = (uint8_t)hb;
        packed[(size_t)b * 2 * nb + nb + j] = (uint8_t)pb;
    }
}

__global__ __launch_bounds__(256) void nastar_unpack_kernel(const uint8_t* __restrict__ packed, float* __restrict__ hist,
                                                            long long* __restrict__ paths, int B, int HW, int nb)
{
    const long long total = (long long)B * nb;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(t / nb), j = (int)(t - (long long)b * nb);
        const uint32_t hb = packed[(size_t)b * 2 * nb + j], pb = packed[(size_t)b * 2 * nb + nb + j];
        const size_t base = (size_t)b * HW + (size_t)j * 8;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (j * 8 + k < HW) {
                hist[base + k] = ((hb >> (7 - k)) & 1u) ? 1.0f : 0.0f;
                paths[base + k] = (pb >> (7 - k)) & 1u;
            }
        }
    }
}


// ---- the reference's stopping step for a batch with maps in the batch-coupled class (differentiable_astar.py:251-252) -------------------
// t_end = the first step at which EVERY map selects its goal: a map that is not marked selects it at every step from its own goal step on
// (fixed point), a marked one at the steps its PROBE bitmap names; without such a step the budget ends the loop (t_end = max_iters - 1).
// tcell = {t_end (-1: no map is marked -- nothing to re-run), number of marked maps, t_max = max over the solved maps of their goal step}.
// ONE workgroup: the bitmaps of the marked maps are AND-ed word by word in LDS (words from t_max on).
constexpr int kTendThreads = 1024;
constexpr int kTendStaticLdsBytes = 16;  // s_tmax, s_nm, s_first below (12 bytes), rounded up
constexpr int kTendMaxLdsWords = (64 * 1024 - kTendStaticLdsBytes) / 4;  // static + dynamic LDS of the launch stay within 64 KiB
__global__ __launch_bounds__(kTendThreads) void nastar_batchloop_tend_kernel(const int* __restrict__ iters, const int* __restrict__ status,
                                                                            const int* __restrict__ marks, const uint32_t* __restrict__ bitmap,
                                                                            int words, int B, int max_iters, int* __restrict__ tcell, int lds_words)
{
    extern __shared__ uint32_t s_and[];
    __shared__ int s_tmax, s_nm;
    __shared__ unsigned s_first;
    const int tid = threadIdx.x;
    if (tid == 0) { s_tmax = -1; s_nm = 0; s_first = 0xFFFFFFFFu; }
    __syncthreads();
    int tmax = -1, nm = 0;
    for (int b = tid; b < B; b += kTendThreads) {
        if (status[b] != NASTAR_OK) continue;  // (the reference crashes on an unsolvable map; here it is reported and takes no part)
        tmax = max(tmax, iters[b] - 1);
        nm += marks[b] != 0;
    }
    if (tmax >= 0) atomicMax(&s_tmax, tmax);
    if (nm) atomicAdd(&s_nm, nm);
    __syncthreads();
    tmax = s_tmax;
    nm = s_nm;
    if (nm == 0 || tmax < 0) {
        if (tid == 0) { tcell[0] = -1; tcell[1] = 0; tcell[2] = tmax; }
        return;
    }
    const int w0 = tmax >> 5, nw = words - w0;
    unsigned first = 0xFFFFFFFFu;
    if (nw <= lds_words) {
        for (int w = tid; w < nw; w += kTendThreads) s_and[w] = 0xFFFFFFFFu;
        __syncthreads();
        const long long total = (long long)B * nw;
        for (long long i = tid; i < total; i += kTendThreads) {
            const int b = (int)(i / nw), w = (int)(i - (long long)b * nw);
            if (marks[b] != 0 && status[b] == NASTAR_OK) atomicAnd(&s_and[w], bitmap[(size_t)b * words + w0 + w]);
        }
        __syncthreads();
        for (int w = tid; w < nw; w += kTendThreads) {
            uint32_t v = s_and[w];
            if (w == 0) v &= 0xFFFFFFFFu << (tmax & 31);
            if (v) first = min(first, (unsigned)((w0 + w) * 32 + __builtin_ctz(v)));
        }
    } else {  // (a budget too long for LDS: each thread ANDs whole columns)
        for (int w = tid; w < nw; w += kTendThreads) {
            uint32_t v = 0xFFFFFFFFu;
            for (int b = 0; b < B; ++b)
                if (marks[b] != 0 && status[b] == NASTAR_OK) v &= bitmap[(size_t)b * words + w0 + w];
            if (w == 0) v &= 0xFFFFFFFFu << (tmax & 31);
            if (v) first = min(first, (unsigned)((w0 + w) * 32 + __builtin_ctz(v)));
        }
    }
    if (first != 0xFFFFFFFFu) atomicMin(&s_first, first);
    __syncthreads();
    if (tid == 0) {
        const unsigned f = s_first;
        tcell[0] = (f < (unsigned)(max_iters - 1)) ? (int)f : max_iters - 1;
        tcell[1] = nm;
        tcell[2] = tmax;
    }
}

}  // namespace nastar
