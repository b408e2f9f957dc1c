// nastar_search_asm5.hip.h -- the round-4 stream (nastar_search_asm4.hip.h, whose sections it reuses) for maps that keep the HEURISTIC
// where the cost word was ("stored_h"): 60 instructions per 32x32 step at g_ratio == 0.5 instead of 71.
//
// VanillaAstar hands ONE binary tensor over as cost map AND obstacle map (reference astar.py:93-94).  Every cell the search can relax
// or key then costs exactly 1.0 (only passable cells are opened, :228-229; a START on an obstacle is the one exception, handled as in
// nastar_search_unit.hip.h: it is opened with g = -1.0, fl(-1.0 + 1.0) = fl(0 + 0)), so the cost word of the 8-byte cell record
// carries no information.  The kernel decides this per map while it loads (nastar_forward_compact_body.inc: cost == passable by
// pointer, every value exactly 0.0 or 1.0, raw-bit keys apply, start and goal exist) and then writes hh = fl(h0 + 1.0) into that
// word for every cell: same bytes per map, same maps per CU, same LDS carve.  In the step
//   * the ten instructions of the heuristic (NASTAR_ASM3_X_HEUR, one of them v_sqrt_f32) and the add of the cost go: the key is
//     f = fl(g + hh) from the (g, hh) pair the cell read delivers anyway;  g2 = fl(g[s*] + 1.0), a 4-byte read of g[s*];
//   * the lanes no longer need (r_l, c_l) before their reads: the cell is (s* & colmask) + delta, two VALU instructions in place of
//     six, bit for bit the index the round-4 prefix forms (out-of-map neighbour lanes keep that garbage index and only READ with it);
//     s* goes into the shift of its byte offset as an SGPR operand (no v_mov);
//   * the in-map test needs nothing from LDS and moves BEHIND the cell read, into the shadow the heuristic leaves.
// In front of the two cell reads the step has 12 instructions instead of 16, behind the wait one fewer.
// CLOSE, WAIT, RELAX, SELECT, the read-back, the exits, the log part and the dive are the round-4 / round-3 sections, token for token.
// Hazard rules as in nastar_search_asm.hip.h.  s42 (s*, written by v_readlane) is now read by a VALU instruction at the head of the
// prefix: s_cmp_eq_u32 + s_cbranch_scc1 of the goal test stand between (2 wait states, the 2 that VALU-written SGPR -> VALU read
// needs; the log part and the dive's way in only add to them).
#pragma once
#include "nastar_search_asm4.hip.h"

namespace nastar {

#define NASTAR_ASM5_X_PREFIX \
        "v_and_b32 v46, s42, %[cmask]\n\t" /* chunk lanes: first cell of the chunk of s*; others: s* */ \
        "v_lshlrev_b32_e64 v27, 3, s42\n\t" \
        "v_add_u32 v46, v46, %[delta]\n\t" /* this lane's cell; garbage on out-of-map neighbour lanes, which only ever READ with it */ \
        "ds_read_b32 v28, v27\n\t" /* g[s*] */ \
        "v_lshlrev_b32 v26, 3, v46\n\t" \
        "v_lshrrev_b32 v50, 4, v46\n\t" \
        "v_lshlrev_b32 v50, 3, v50\n\t" /* byte offset of cmin[chunk of this lane's cell] */
#define NASTAR_ASM5_X_READCELL \
        "ds_read_b64 v[30:31], v26\n\t" /* g[il], hh[il] = fl(h0 + 1.0) */
#define NASTAR_ASM5_X_INMAP \
 /* conv2d zero padding (:77-93), in the shadow of the LDS round trip */ \
        "s_lshr_b32 s43, s42, %[LOGW]\n\t" /* r* */ \
        "s_and_b32 s44, s42, %[WM1]\n\t" /* c* */ \
        "v_add_u32 v32, s43, %[dr]\n\t" /* r_l */ \
        "v_and_b32 v33, s44, %[cmask]\n\t" \
        "v_add_u32 v33, v33, %[dcc]\n\t" /* c_l */ \
        "v_max_u32 v23, v32, v33\n\t" \
        "v_cmp_gt_u32 vcc, %[W], v23\n\t" /* inside the map; true for lane 8 and the chunk lanes */ \
        "s_and_b64 s[54:55], vcc, %[mnb]\n\t" /* in-map neighbour lanes */
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
        : [it] "+s"(it), [sel] "=s"(sel), [mkey] "=s"(mkey) \
        : [l8] "v"(v_l8), [dr] "v"(v_dr), [cmask] "v"(v_cmask), [dcc] "v"(v_dcc), [delta] "v"(v_delta), [pcode] "v"(v_pcode), \
          [cls] "v"(v_cls), [vminf] "v"(v_minf), [goal] "s"(goal_idx), \
          [maxit] "s"(max_iters), [cgr] "s"(cgr), [comg] "s"(comg), [csq] "s"(csq), [crcp] "s"(rcp_sqrtW), \
          [mnb] "s"(m_nb), [logp] "s"(logp), \
          [CMIN] "i"(CMIN), [CMIN16] "i"(CMIN + 16), [PDIR] "i"(PDIR), [LOGW] "i"(LOGW), [WM1] "i"((1 << LOGW) - 1), [W] "i"(1 << LOGW) \
        : "memory", "vcc", "scc", "v20", "v21", "v22", "v23", "v26", "v27", "v28", "v30", "v31", "v32", "v33", \
          "v40", "v41", "v42", "v43", "v46", "v47", "v48", "v49", "v50", "s40", "s41", "s42", \
          "s43", "s44", "s54", "s55", "s53", "v53", "v54", "v12", "v13", "v14", "v15", "v16", "v17", "v18", "v19", "s48", "s49", \
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
    constexpr int CMIN = LG::CMIN;
    constexpr int PDIR = LG::PDIR;
    static_assert((CPL == 1 || CPL == 4) && LG::HW >= 256, "1 or 4 chunk minima per lane, chunks inside one map row");
    int dr, dc;
    neighbour_delta(lane & 7, dr, dc);
    const bool is_nb = lane < 8, is_chk = (lane & 48) == 16;
    const int v_dr = is_nb ? dr : 0;
    const int v_dcc = is_nb ? dc : (is_chk ? (lane & 15) : 0);
    const int v_delta = is_nb ? dr * (1 << LOGW) + dc : (is_chk ? (lane & 15) : 0);
    const uint32_t v_cmask = is_chk ? 0xFFFFFFF0u : 0xFFFFFFFFu;
    const uint32_t v_cls = is_chk ? 0x1F8u : 0u;  // finite = open
    const uint32_t v_pcode = P_PASS | (uint32_t)(lane & 7);
    const uint32_t v_l8 = (uint32_t)lane * 8u * CPL;
    const float v_minf = NASTAR_NEG_INF;
    const unsigned long long m_nb = 0xFFull;
    int it = __builtin_amdgcn_readfirstlane(iters);
    goal_idx = __builtin_amdgcn_readfirstlane(goal_idx);
    max_iters = __builtin_amdgcn_readfirstlane(max_iters);
    int sel;
    uint32_t mkey = 0;
    unsigned long long logp = reinterpret_cast<unsigned long long>(log_row);
#define NASTAR_A5_EXPAND(MH, MG, SET55) \
    NASTAR_ASM5_X_PREFIX NASTAR_ASM3_X_CLOSE NASTAR_ASM5_X_READCELL NASTAR_ASM5_X_INMAP NASTAR_ASM3_X_WAIT NASTAR_ASM5_X_KEY(MH, MG) \
        NASTAR_ASM3_X_RELAX(SET55)
    /* entry -> select -> [log] expand, prefetch -> budget test -> select ... */
#define NASTAR_A5_BODY(N, MH, MG, LOGPART) \
    NASTAR_ASM4_ENTRY NASTAR_ASM_READ_##N NASTAR_ASM_LOOPTOP NASTAR_ASM_LOCALMIN_##N NASTAR_ASM4_SELECT LOGPART NASTAR_A5_EXPAND(MH, MG, ) \
        NASTAR_ASM_READ_##N NASTAR_ASM4_LOOPEND
    /* entry -> select; [dive lookup ->] selected: log, expand, prefetch, budget + dive test -> dive | select -> selected */
#define NASTAR_A5_BODY_DIVE(N, MH, MG, LOGPART) \
    NASTAR_ASM4_ENTRY NASTAR_ASM_READ_##N "s_branch .Lsel%=\n" NASTAR_ASM4_DIVE_LOOKUP LOGPART \
        NASTAR_A5_EXPAND(MH, MG, "v_cmp_lt_u32_e64 s[60:61], v47, s40\n\t") NASTAR_ASM_READ_##N NASTAR_ASM3_DIVE_TEST ".Lsel%=:\n\t" \
        "s_waitcnt lgkmcnt(0)\n\t" NASTAR_ASM_LOCALMIN_##N NASTAR_ASM4_SELECT "s_branch .Lselected%=\n" NASTAR_ASM4_EXITS
#define NASTAR_A5_RUN2(BODY, N, MH, MG) \
    do { \
        if constexpr (kLog) asm volatile(BODY(N, MH, MG, NASTAR_ASM3_LOG) NASTAR_ASM5_OPERANDS); \
        else asm volatile(BODY(N, MH, MG, ) NASTAR_ASM5_OPERANDS); \
    } while (0)
#define NASTAR_A5_RUN(BODY, N) \
    do { \
        if constexpr (kHalf) NASTAR_A5_RUN2(BODY, N, , ); \
        else NASTAR_A5_RUN2(BODY, N, NASTAR_ASM5_MULH, NASTAR_ASM5_MULG); \
    } while (0)
    if constexpr (CPL == 1 && kDive) NASTAR_A5_RUN(NASTAR_A5_BODY_DIVE, 1);
    else if constexpr (CPL == 1) NASTAR_A5_RUN(NASTAR_A5_BODY, 1);
    else if constexpr (kDive) NASTAR_A5_RUN(NASTAR_A5_BODY_DIVE, 4);
    else NASTAR_A5_RUN(NASTAR_A5_BODY, 4);
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
