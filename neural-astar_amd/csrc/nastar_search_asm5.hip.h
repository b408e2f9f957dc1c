// nastar_search_asm5.hip.h -- the round-4 stream (nastar_search_asm4.hip.h, whose sections it reuses) for maps that keep the HEURISTIC
// where the cost word was ("stored_h"): 51 instructions per 32x32 step at g_ratio == 0.5 (55 before the row-wide chunks, below), the general stream 67.
//
// VanillaAstar hands ONE binary tensor over as cost map AND obstacle map (reference astar.py:93-94).  Every cell the search can relax
// or key then costs exactly 1.0 (only passable cells are opened, :228-229; a START on an obstacle is the one exception, handled as in
// nastar_search_unit.hip.h: it is opened with g = -1.0, fl(-1.0 + 1.0) = fl(0 + 0)), so the cost word of the 8-byte cell record
// carries no information.  The kernel decides this per map while it loads (nastar_forward_compact_body.inc: cost == passable by
// pointer, every value exactly 0.0 or 1.0, raw-bit keys apply, start and goal exist) and then writes hh = fl(h0 + 1.0) into that
// word for every cell: same bytes per map, same maps per CU, same LDS carve.  In the step
//   * the ten instructions of the heuristic (NASTAR_ASM3_X_HEUR, one of them v_sqrt_f32) and the add of the cost go: the key is
//     f = fl(g + hh) from the (g, hh) pair the cell read delivers anyway;  g2 = fl(g[s*] + 1.0), a 4-byte read of g[s*];
//   * the lanes need no (r_l, c_l) at all: the cell is (s* & colmask) + delta, two VALU instructions in place of six;  s* goes into
//     the shift of its byte offset as an SGPR operand (no v_mov);
//   * conv2d's zero padding (:77-93) is not computed, the map geometry fixes it.  COLUMNS: which neighbour lanes leave the map depends
//     on c* alone, and c* is the low bits of s*: a loop-invariant VGPR holds in lane L the 8-bit mask of the neighbour lanes that stay
//     inside for c* = L & (W - 1), and ONE v_readlane_b32 with s* as the lane select (the instruction takes it modulo 64: lane
//     (r* & 1, c*) at 32x32, c* at 64x64, (r* & 3, c*) at 16x16) yields the low half of the relaxation's EXEC mask; the high half is
//     zeroed once in the block's entry.  ROWS: the layout has a guard row of W cells on either side of gc[] whose g words are -inf
//     (AsmLayout, carve_compact_asm_lds).  With its column inside the map, a neighbour lane of row -1 or row W reads a guard cell, and
//     "g[n] > g2" fails on -inf for every g2 -- the blocked start's 0.0 included -- as it does on a closed cell: the lane never writes.
//     A lane whose column is outside reads a cell of the neighbouring row (or a guard cell, or garbage in front of / behind the state)
//     and is not in the EXEC mask.  One instruction in place of eight;
//   * lane 8's reset of the chunk entry moves behind the cell read with the two instructions of the chunk offset: it only has to
//     precede this step's ds_min_u64, and a wave's LDS operations stay in order.  The cell read's shadow thus keeps six instructions
//     (lookup, chunk offset, reset).  The wait in front of the key is s_waitcnt lgkmcnt(1): LDS operations return in order, so it
//     covers the two reads and the close and NOT the reset behind them -- with lgkmcnt(0) the reset's write latency lands on every
//     step's critical path and the step is slower than the one it replaces (measured: DESIGN.md 4.1, profiles/guard_rows.json).
// In front of the cell read the step has 8 instructions instead of 11, behind it six that cover its round trip, behind the wait as
// many as before: 55 per 32x32 step at g_ratio == 0.5 instead of 60.
// ROW-WIDE CHUNKS (32x32): a chunk minimum covers a whole map row (AsmLayout::CCL = 5; cmin[] keeps 64 entries, 32..63 idle for good), so
// the 32 live minima sit in lanes 0-31, two DPP rows, and the selection needs no stage across four rows: behind row_mirror it ends with
//     s_add_u32 it, it, 1 | v_readlane_b32 s40, v22, 0 | v_readlane_b32 s53, v22, 16 | s_min_u32 s40, s40, s53
// (NASTAR_ASM4_FIN_2) where the four-row finish has eight instructions (two row_bcast stages, three s_nop around them, the v_readlane
// of lane 63, the counter, one more s_nop): 51 per step instead of 55.  s40 is SALU-written, so the pick's v_cmp_eq_u32 follows at once.
// The chunk lanes are lanes 32-63, cell (s* & ~31) | (lane & 31); lanes 9-31 idle (cell s*, class mask 0).  The lowest lane with the
// minimal key is the lowest row, and a row's entry names its lowest minimal cell (ds_min_u64 on (key, cell)): the first flat index, as
// before.  16x16 has 16 live minima in one DPP row with the 16-cell chunks it always had and ends with one v_readlane (50 per step);
// 64x64 keeps the four-row finish and its machine code.
// RELAX, SELECT's stages, the read-back, the exits, the log part and the dive are the round-4 / round-3 sections, token for token.
// Hazard rules as in nastar_search_asm.hip.h.  s42 (s*, written by v_readlane) is read by a VALU instruction at the head of the
// prefix: s_cmp_eq_u32 + s_cbranch_scc1 of the goal test stand between (2 wait states, the 2 that VALU-written SGPR -> VALU read
// needs; the log part and the dive's way in only add to them), and as a LANE SELECT nine instructions later (4 wait states needed).
// s54 is VALU-written (v_readlane) and read by a scalar instruction only (s_mov_b64 exec), ten instructions later: no rule applies.
#pragma once
#include "nastar_search_asm4.hip.h"

namespace nastar {

#define NASTAR_ASM5_ENTRY \
        "s_mov_b32 s55, 0\n\t" /* high half of the relaxation's EXEC mask s[54:55]: neighbour lanes are lanes 0-7 */
#define NASTAR_ASM5_X_PREFIX \
        "v_and_b32 v46, s42, %[cmask]\n\t" /* chunk lanes: first cell of the chunk of s*; others: s* */ \
        "v_lshlrev_b32_e64 v27, 3, s42\n\t" \
        "v_add_u32 v46, v46, %[delta]\n\t" /* this lane's cell; a guard cell or garbage on out-of-map neighbour lanes, which only ever READ with it */ \
        "ds_read_b32 v28, v27 offset:%[GC]\n\t" /* g[s*] */ \
        "v_lshlrev_b32 v26, 3, v46\n\t"
#define NASTAR_ASM5_X_CLOSE \
 /* lane 8 closes s* (:222-225) BEFORE the lanes read their cells.  (All 64 lanes storing the wave-uniform value without the two EXEC \
    writes is 1.7 ns faster on the lone step and 1.3 % slower on the headline batch: measured) */ \
        "s_mov_b64 exec, 0x100\n\t" \
        "ds_write_b32 v27, %[vminf] offset:%[GC]\n\t" \
        "s_mov_b64 exec, -1\n\t"
#define NASTAR_ASM5_X_READCELL \
        "ds_read_b64 v[30:31], v26 offset:%[GC]\n\t" /* g[il], hh[il] = fl(h0 + 1.0) */
#define NASTAR_ASM5_X_SHADOW \
 /* in the shadow of the LDS round trip: conv2d's zero padding (:77-93) for the COLUMNS -- lane (s* & 63) of colmask holds the neighbour \
    lanes whose column stays inside the map for c* = s* & (W - 1); v_readlane_b32 takes the lane select modulo 64 -- the chunk offset, \
    and lane 8 (whose cell is s*) empties the entry of the chunk of s*: ahead of this step's ds_min_u64, a wave's LDS operations stay in order */ \
        "v_readlane_b32 s54, %[colmask], s42\n\t" \
        "v_lshrrev_b32 v50, %[CCL], v46\n\t" \
        "v_lshlrev_b32 v50, 3, v50\n\t" /* byte offset of cmin[chunk of this lane's cell] */ \
        "s_mov_b64 exec, 0x100\n\t" \
        "ds_write_b64 v50, v[48:49] offset:%[CMIN]\n\t" \
        "s_mov_b64 exec, -1\n\t"
#define NASTAR_ASM5_X_WAIT \
        "s_waitcnt lgkmcnt(1)\n\t" /* LDS operations return in order: all but the reset above, which nothing here waits for */
#define NASTAR_ASM5_X_KEY(MULH, MULG) \
        "v_add_f32 v40, 1.0, v28\n\t" /* :234 g2 = g[s*] + cost[s*], cost[s*] = 1.0 */ \
        MULH /* :206 (1-g_ratio)*h */ \
        "v_cndmask_b32_e64 v41, v30, v40, %[mnb]\n\t" /* neighbour lanes key g2, chunk lanes their own g */ \
        MULG /* :206 g_ratio*g */ \
        "v_add_f32 v41, v41, v31\n\t" /* :206 f */ \
        "v_mul_f32 v42, %[crcp], v41\n\t" /* :207 f / sqrt(W), correctly rounded (tools/fastdiv_check.c) */ \
        "v_fma_f32 v43, -v42, %[csq], v41\n\t" \
        "v_fma_f32 v47, v43, %[crcp], v42\n\t" /* q >= +0: its bits are the key; [v46:v47] = (cell, key) */
#define NASTAR_ASM5_MULH "v_mul_f32 v31, %[comg], v31\n\t"
#define NASTAR_ASM5_MULG "v_mul_f32 v41, %[cgr], v41\n\t"

#define NASTAR_ASM5_OPERANDS \
        : [it] "+&s"(it), [sel] "=s"(sel), [mkey] "=s"(mkey) \
        : [l8] "v"(v_l8), [cmask] "v"(v_cmask), [colmask] "v"(v_colmask), [delta] "v"(v_delta), [pcode] "v"(v_pcode), \
          [cls] "v"(v_cls), [vminf] "v"(v_minf), [goal] "s"(goal_idx), \
          [maxit] "s"(max_iters), [cgr] "s"(cgr), [comg] "s"(comg), [csq] "s"(csq), [crcp] "s"(rcp_sqrtW), \
          [mnb] "s"(m_nb), [logp] "s"(logp), \
          [GC] "i"(GC), [CMIN] "i"(CMIN), [CMIN16] "i"(CMIN + 16), [PDIR] "i"(PDIR), [CCL] "i"(LG::CCL) \
        : "memory", "vcc", "scc", "v20", "v21", "v22", "v23", "v26", "v27", "v28", "v30", "v31", \
          "v40", "v41", "v42", "v43", "v46", "v47", "v48", "v49", "v50", "s40", "s41", "s42", \
          "s54", "s55", "s53", "v53", "v54", "v12", "v13", "v14", "v15", "v16", "v17", "v18", "v19", "s48", "s49", \
          "s50", "s51", "v55", "v56", "v57", "s56", "s58", "s59", "s60", "s61"

// Contract of search_loop_asm4 on the compact layout, with these preconditions on top: gc[i].y = fl(h0(i) + 1.0f) for every cell i
// (compact_store_heuristic below), every cell that can be relaxed costs 1.0, and a start that sits on an obstacle was opened with
// g = -1.0.  kHalf: g_ratio == 0.5 exactly (the start's key formed by compact_open_start with half_key).
template <int LOGW, bool kLog, bool kDive, bool kHalf>
__device__ __forceinline__ int search_loop_asm5(float cgr, float comg, float csq, int lane, int goal_idx, int max_iters, int& iters,
                                                float rcp_sqrtW, int* log_row)
{
    using LG = AsmLayout<LOGW>;
    constexpr int CPL = LG::CPL;
    constexpr int GC = LG::GC;
    constexpr int CMIN = LG::CMIN;
    constexpr int PDIR = LG::PDIR;
    constexpr int ROWS = LG::ROWS;
    static_assert((CPL == 1 || CPL == 4) && LG::HW >= 256 && (1 << LG::CCL) <= LG::W, "1 or 4 chunk minima per lane, chunks inside one map row");
    int dr, dc;
    neighbour_delta(lane & 7, dr, dc);
    // chunk lanes: lanes 16-31, or lanes 32-63 where a chunk is a 32-cell map row: cell (s* & ~31) | (lane & 31)
    const bool is_nb = lane < 8, is_chk = ROWS == 2 ? lane >= 32 : (lane & 48) == 16;
    const int v_delta = is_nb ? dr * (1 << LOGW) + dc : (is_chk ? (lane & ((1 << LG::CCL) - 1)) : 0);
    const uint32_t v_cmask = is_chk ? ~((1u << LG::CCL) - 1u) : 0xFFFFFFFFu;
    const uint32_t v_cls = is_chk ? 0x1F8u : 0u;  // finite = open
    const uint32_t v_pcode = P_PASS | (uint32_t)(lane & 7);
    const uint32_t v_l8 = (uint32_t)lane * 8u * CPL;
    const float v_minf = NASTAR_NEG_INF;
    const unsigned long long m_nb = 0xFFull;
    // lane L: the neighbour lanes (bit j = lane j, the order of neighbour_delta: dc = -1 on lanes 0, 3, 5, dc = +1 on lanes 2, 4, 7) whose
    // column stays inside the map when s* sits in column L & (W - 1); the step reads it at lane s* & 63
    const int col = lane & ((1 << LOGW) - 1);
    const uint32_t v_colmask = 0xFFu & ~(col == 0 ? 0x29u : 0u) & ~(col == (1 << LOGW) - 1 ? 0x94u : 0u);
    int it = __builtin_amdgcn_readfirstlane(iters);
    goal_idx = __builtin_amdgcn_readfirstlane(goal_idx);
    max_iters = __builtin_amdgcn_readfirstlane(max_iters);
    int sel;
    uint32_t mkey = 0;
    unsigned long long logp = reinterpret_cast<unsigned long long>(log_row);
#define NASTAR_A5_EXPAND(MH, MG, SET55) \
    NASTAR_ASM5_X_PREFIX NASTAR_ASM5_X_CLOSE NASTAR_ASM5_X_READCELL NASTAR_ASM5_X_SHADOW NASTAR_ASM5_X_WAIT NASTAR_ASM5_X_KEY(MH, MG) \
        NASTAR_ASM3_X_RELAX(SET55)
    /* entry -> select -> [log] expand, prefetch -> budget test -> select ... */
#define NASTAR_A5_BODY(N, MH, MG, FIN, LOGPART) \
    NASTAR_ASM5_ENTRY NASTAR_ASM4_ENTRY NASTAR_ASM_READ_##N NASTAR_ASM_LOOPTOP NASTAR_ASM_LOCALMIN_##N NASTAR_ASM4_SELECT(FIN) LOGPART NASTAR_A5_EXPAND(MH, MG, ) \
        NASTAR_ASM_READ_##N NASTAR_ASM4_LOOPEND
    /* entry -> select; [dive lookup ->] selected: log, expand, prefetch, budget + dive test -> dive | select -> selected */
#define NASTAR_A5_BODY_DIVE(N, MH, MG, FIN, LOGPART) \
    NASTAR_ASM5_ENTRY NASTAR_ASM4_ENTRY NASTAR_ASM_READ_##N "s_branch .Lsel%=\n" NASTAR_ASM4_DIVE_LOOKUP LOGPART \
        NASTAR_A5_EXPAND(MH, MG, "v_cmp_lt_u32_e64 s[60:61], v47, s40\n\t") NASTAR_ASM_READ_##N NASTAR_ASM3_DIVE_TEST ".Lsel%=:\n\t" \
        "s_waitcnt lgkmcnt(0)\n\t" NASTAR_ASM_LOCALMIN_##N NASTAR_ASM4_SELECT(FIN) "s_branch .Lselected%=\n" NASTAR_ASM4_EXITS
#define NASTAR_A5_RUN2(BODY, N, MH, MG, FIN) \
    do { \
        if constexpr (kLog) asm volatile(BODY(N, MH, MG, FIN, NASTAR_ASM3_LOG) NASTAR_ASM5_OPERANDS); \
        else asm volatile(BODY(N, MH, MG, FIN, ) NASTAR_ASM5_OPERANDS); \
    } while (0)
#define NASTAR_A5_RUN(BODY, N, FIN) \
    do { \
        if constexpr (kHalf) NASTAR_A5_RUN2(BODY, N, , , FIN); \
        else NASTAR_A5_RUN2(BODY, N, NASTAR_ASM5_MULH, NASTAR_ASM5_MULG, FIN); \
    } while (0)
    /* the finish of the selection by the rows of live chunk minima (nastar_search_asm4.hip.h) */
#define NASTAR_A5_RUN_ROWS(BODY) \
    do { \
        if constexpr (CPL == 4) NASTAR_A5_RUN(BODY, 4, NASTAR_ASM4_FIN_4); \
        else if constexpr (ROWS == 4) NASTAR_A5_RUN(BODY, 1, NASTAR_ASM4_FIN_4); \
        else if constexpr (ROWS == 2) NASTAR_A5_RUN(BODY, 1, NASTAR_ASM4_FIN_2); \
        else NASTAR_A5_RUN(BODY, 1, NASTAR_ASM4_FIN_1); \
    } while (0)
    if constexpr (kDive) NASTAR_A5_RUN_ROWS(NASTAR_A5_BODY_DIVE);
    else NASTAR_A5_RUN_ROWS(NASTAR_A5_BODY);
#undef NASTAR_A5_RUN_ROWS
#undef NASTAR_A5_RUN
#undef NASTAR_A5_RUN2
#undef NASTAR_A5_BODY_DIVE
#undef NASTAR_A5_BODY
#undef NASTAR_A5_EXPAND
    iters = it;
    return (sel >= 0 && mkey == 0xFFFFFFFFu) ? -1 : sel;
}

// gc[i].y = fl(h0(i) + 1.0f) for every cell of a stored_h map, all 64 lanes, HW / 64 cells each (lane l owns cells l + 64 k: one
// column, every (64 / W)-th row).  The arithmetic is the integer formulation of NASTAR_ASM3_X_HEUR, instruction for instruction
// (|dr|, |dc|, Chebyshev = max, dr^2 + dc^2 exact in u32, two converts, the bare v_sqrt_f32 -- exact for sides < 140 --, one rounding
// per fp32 op), so a stored value has the bits the general stream computes in its step.
template <int LOGW>
__device__ __forceinline__ void compact_store_heuristic(const CompactLds& l, int lane, int goal_r, int goal_c)
{
    constexpr int W = 1 << LOGW, HW = W * W;
    static_assert(W <= 64 && HW % 64 == 0, "a lane's cells share one column");
    const int c = lane & (W - 1);
    const int dcol = c > goal_c ? c - goal_c : goal_c - c;
    const uint32_t dc2 = (uint32_t)(dcol * dcol);
#pragma unroll 4
    for (int k = 0; k < HW / 64; ++k) {
        const int i = lane + 64 * k;
        const int r = i >> LOGW;
        const int drow = r > goal_r ? r - goal_r : goal_r - r;
        const uint32_t cheb = (uint32_t)(drow > dcol ? drow : dcol);
        const float euc = __builtin_amdgcn_sqrtf((float)((uint32_t)(drow * drow) + dc2));
        const float h0 = (float)cheb + 0.001f * euc;
        l.gc[i].y = h0 + 1.0f;
    }
}

}  // namespace nastar
