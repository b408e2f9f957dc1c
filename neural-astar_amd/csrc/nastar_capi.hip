// nastar_capi.hip -- the C ABI declared in include/nastar.h (libnastar_hip.so): argument checks and kernel choice.  Host code only: the
// kernels it launches are in nastar_search_kernels.hip.h and the headers that one builds on.
// gfx950 only.  Build: see neural-astar_amd/csrc/Makefile (hipcc --offload-arch=gfx950 -ffp-contract=off).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <stddef.h>
#include <time.h>

#include "nastar_host.hip.h"
#include "nastar_search.hip.h"
#include "nastar_search_hybrid.hip.h"
#include "nastar_search_compact.hip.h"
#include "nastar_search_asm.hip.h"
#ifdef NASTAR_DEV
#include "nastar_dev_flags.h"  // A/B switches of the development build (make dev): round-3 / round-2 streams, no dive, compiled step
#endif
#include "nastar_search_asm4.hip.h"  // (reuses the instruction sections of nastar_search_asm3.hip.h; the round-3 LOOP itself is only instantiated by the development build)
#include "nastar_search_asm5.hip.h"  // (the round-4 stream for maps that keep the heuristic where the cost word was)
#include "nastar_search_unit.hip.h"
#include "nastar_placement.hip.h"
#include "nastar_backward_replay.hip.h"
#include "nastar_backward_replay_asm.hip.h"
#include "nastar_routes.hip.h"
#include "../../include/nastar_routes.h"
#include "../../include/nastar_sources.h"
#include "../../include/nastar_levels.h"
#include "nastar_search_kernels.hip.h"
#include "nastar_ticket.hip.h"

namespace nastar {

thread_local char g_last_error[256] = "";

// maps whose state lives in HBM: three levels (cell -> chunk minimum per 64 cells -> super-chunk minimum per 64 chunks), the two minima arrays in
// LDS: 8 B per 64 cells must fit one CU -- 1,179,648 cells (1024 x 1152; 1024 x 1024 takes 130 KiB)
constexpr long long kMaxGlobalCells = 1179648;
// from 6400 cells (80 x 80) on the large-map kernel is the faster one although the compact state would still fit LDS up to ~17 k cells: the
// compiled LDS loop scans HW / 1024 chunk entries per lane and step and keeps 1-2 maps resident per CU; the hybrid step (0.66-0.68 us since its
// next selection travels in scalar registers, nastar_search_hybrid.hip.h) does not grow with the map and keeps 32 maps resident per CU.
// Measured (tools/probe_large.py mid, profiles/r06/probe_mid.jsonl; hybrid / LDS launch time, one map .. 1024 maps): 72x72 0.9-1.33,
// 80x80 0.76-1.01, 96x96 0.76-1.05, 112x112 0.50-0.82, 128x128 0.41-0.58.
constexpr long long kHybridFromCells = 6400;
constexpr size_t kOrderCheckBytes = 16;                // NASTAR_FLAG_CHECK_ORDER: verdict word at the end of the workspace

// maps one launch keeps resident at once: LDS bytes per map against 160 KiB per CU (and 32 wavefront slots), times the CUs of the device
static long long resident_capacity(size_t lds_per_map)
{
    // CU count of the CURRENT device, looked up once per device (a launch on device 3 must not size itself by device 0's answer)
    static int cus_of[64] = {0};
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64) {
        int n = __atomic_load_n(&cus_of[dev], __ATOMIC_RELAXED);
        if (n == 0) {
            if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
            __atomic_store_n(&cus_of[dev], n, __ATOMIC_RELAXED);  // (racing threads store the same value)
        }
        cus = n;
    }
    long long per_cu = (long long)(kMaxLdsBytes / (lds_per_map ? lds_per_map : 1));
    if (per_cu > 32) per_cu = 32;
    if (per_cu < 1) per_cu = 1;
    return per_cu * cus;
}

static int make_cdims(int B, int H, int W, int max_iters, double g_ratio, CompactDims& d)
{
    if (B <= 0 || H <= 0 || W <= 0 || max_iters <= 0) return NASTAR_ERR_BAD_SHAPE;
    if (H > 65535 || W > 65535 || (long long)H * W > 65535 - CCSZ) return NASTAR_ERR_UNSUPPORTED;
    d.H = H;
    d.W = W;
    d.HW = H * W;
    d.nchunks = (d.HW + CCSZ - 1) / CCSZ;
    d.HWp = d.nchunks * CCSZ;
    d.CPL = (d.nchunks + 63) / 64;
    d.NCp = d.CPL * 64;
    d.magicW = (uint32_t)((1ull << 32) / (unsigned)W) + 1u;
    d.gr = (float)g_ratio;
    d.omg = (float)(1.0 - g_ratio);  // python evaluates (1 - g_ratio) in double, ATen casts the scalar to fp32
    d.sqrtW = (float)sqrt((double)W);  // math.sqrt(W) in double, then the fp32 scalar of the division (:207)
    return NASTAR_OK;
}

// maps whose compact state (9 B/cell, nastar_search_compact.hip.h) does not fit the 160 KiB of one CU keep it in HBM
// cells from which a map takes the large-map kernel although its compact state would still fit LDS (the compiled LDS loop scans CPL = HW / 1024
// chunk entries per lane and step; the hybrid kernel's step does not grow with the map).  NASTAR_HYBRID_FROM_CELLS overrides it (probes).
static long long hybrid_from_cells()
{
    static long long v = -1;
    if (v < 0) {
        const char* e = getenv("NASTAR_HYBRID_FROM_CELLS");
        v = (e && *e) ? atoll(e) : kHybridFromCells;
        if (v < 4097) v = 4097;  // (the hand-scheduled 64x64 stream and everything below it stay LDS-resident)
    }
    return v;
}

static bool needs_global_state(int H, int W)
{
    const long long HW = (long long)H * W;
    if (HW >= hybrid_from_cells()) return true;
    if (HW > 65535 - CCSZ) return true;
    const long long nchunks = (HW + CCSZ - 1) / CCSZ;
    return compact_launch_lds_bytes(H, W, (int)(nchunks * CCSZ), (int)(((nchunks + 63) / 64) * 64), true) > kMaxLdsBytes;
}

// Workspace of a forward launch: [hybrid slabs (maps larger than LDS)] [marks: B int32 + the t_end cell, NASTAR_FLAG_MARK_COUPLED]
// [verdict word of NASTAR_FLAG_CHECK_ORDER].  The probe bitmaps of nastar_forward_batchloop_finish follow at a FIXED offset (as if both flags
// had been given), so that the finish call finds the marks wherever the first launch put them.
struct WsLayout {
    size_t slabs, marks_off, tcell_off, chk_off, total;
};
static WsLayout ws_layout(int B, int H, int W, int flags)
{
    WsLayout l{};
    l.slabs = needs_global_state(H, W) ? (size_t)B * hybrid_slab_bytes(H * W) : 0;
    size_t off = l.slabs;
    if (flags & NASTAR_FLAG_MARK_COUPLED) {
        l.marks_off = off;
        off += ((size_t)B * 4 + 15) & ~(size_t)15;
        l.tcell_off = off;
        off += 16;
    }
    if (flags & NASTAR_FLAG_CHECK_ORDER) {
        l.chk_off = off;
        off += kOrderCheckBytes;
    }
    l.total = off;
    return l;
}
static int bitmap_words_for(int max_iters) { return (max_iters + 31) / 32; }

// flag bits this build understands (the A/B switches exist in the development build only: csrc/nastar_dev_flags.h)
#ifdef NASTAR_DEV
constexpr int kKnownFlags = NASTAR_FLAG_UNIT_COST | NASTAR_FLAG_CHECK_ORDER | NASTAR_FLAG_LOCKSTEP | NASTAR_FLAG_MARK_COUPLED | NASTAR_FLAG_NO_ASM |
                            NASTAR_FLAG_ASM_V2 | NASTAR_FLAG_ASM_V3 | NASTAR_FLAG_NO_DIVE;
#else
constexpr int kKnownFlags = NASTAR_FLAG_UNIT_COST | NASTAR_FLAG_CHECK_ORDER | NASTAR_FLAG_LOCKSTEP | NASTAR_FLAG_MARK_COUPLED;
constexpr int NASTAR_FLAG_NO_ASM = 0, NASTAR_FLAG_ASM_V2 = 0, NASTAR_FLAG_ASM_V3 = 0, NASTAR_FLAG_NO_DIVE = 0;  // (host-side tests below fold away)
#endif

// a neighbor_filter mask of the masked entry points: weights in {0, 1} over the 3x3 cells, the centre cell (bit 4) clear
static bool neighbor_mask_valid(unsigned m) { return (m & ~0x1FFu) == 0u && (m & 0x10u) == 0u; }

// the neighbourhood of a launch: the Moore-8 stencil of the plain kernels, or (the _masked entry points) a neighbor_filter's mask, searched by
// the masked twin of each kernel for EVERY mask, Moore-8 included
// h0: the caller's heuristic maps (the _heuristic entry points; they always take a mask), searched by the third twin of each kernel
struct Neighbourhood {
    bool masked = false;
    uint32_t mask = NASTAR_NEIGHBORS_MOORE8;
    const float* h0 = nullptr;
    bool multi = false;  // include/nastar_sources.h: every non-zero cell of the start map is a source (the fourth and fifth twin of each kernel)
};

// map widths for which the FMA-based division by fl32(sqrt(W)) was verified bit-exact against IEEE division for
// every fp32 f in [2^-100, FLT_MAX] (tools/fastdiv_check.c); widths whose sqrt is a power of two divide exactly.
static bool fastdiv_verified(int W)
{
    static const int ok[] = {2, 8, 32, 128, 512, 10, 12, 20, 24, 28, 40, 45, 48, 50, 60, 96, 100,  // exhaustively checked
                             1, 4, 16, 64, 256, 1024};                                             // sqrt(W) is a power of two
    for (int w : ok)
        if (w == W) return true;
    return false;
}

// kKind: 0 = Moore-8, 1 = masked, 2 = masked with a caller-supplied heuristic, 3 / 4 = the multi-source forms of 1 / 2
template <int kKind, bool kVec4, int LOGW, int LOGH, int CPL_T, bool kFastDiv, bool kLog>
static auto compiled_compact_kernel()
{
    if constexpr (kKind >= 3) return &nastar_forward_compact_sources_kernel<kVec4, LOGW, LOGH, CPL_T, kFastDiv, kLog, kKind == 4>;
    else if constexpr (kKind == 2) return &nastar_forward_compact_heuristic_kernel<kVec4, LOGW, LOGH, CPL_T, kFastDiv, kLog>;
    else if constexpr (kKind == 1) return &nastar_forward_compact_masked_kernel<kVec4, LOGW, LOGH, CPL_T, kFastDiv, kLog>;
    else return &nastar_forward_compact_kernel<kVec4, LOGW, LOGH, CPL_T, kFastDiv, kLog>;
}

// THE decision whether a launch takes a hand-scheduled instantiation (kKind as below; use_asm: Moore-8, no lock-step, not switched off).
// forward_lds asks once and hands the answer on: the kernel (compact_kernel, the ranked kernels) and the launch's dynamic-LDS size
// (compact_launch_lds_bytes: those instantiations carve guard rows) both follow it.
static bool takes_asm_stream(const CompactDims& d, int kind, bool vec4, bool fast, bool use_asm)
{
    return kind == 0 && use_asm && vec4 && fast && compact_asm_shape(d.H, d.W);
}

// the compact-state kernel for a map: a hand-scheduled stream where one exists (Moore-8 only: the streams hard-wire the stencil), else the
// compiled step loop -- compile-time sizes for 16x16, 32x32 and 64x64, one chunk minimum per lane, or runtime sizes
// asm_stream: the answer of takes_asm_stream for this launch (false for every kKind but 0)
template <int kKind, bool kLog>
static auto compact_kernel(const CompactDims& d, bool vec4, bool fast, bool asm_stream)
{
    if constexpr (kKind == 0) {
        if (asm_stream && d.W == 32) return &nastar_forward_compact_kernel<true, 5, 5, 1, true, kLog, true>;
        if (asm_stream && d.W == 16) return &nastar_forward_compact_kernel<true, 4, 4, 1, true, kLog, true>;
        if (asm_stream && d.W == 64) return &nastar_forward_compact_kernel<true, 6, 6, 4, true, kLog, true>;
    }
    if (vec4 && fast && d.H == 32 && d.W == 32) return compiled_compact_kernel<kKind, true, 5, 5, 1, true, kLog>();
    if (vec4 && fast && d.H == 64 && d.W == 64) return compiled_compact_kernel<kKind, true, 6, 6, 4, true, kLog>();
    if (vec4 && fast && d.H == 16 && d.W == 16) return compiled_compact_kernel<kKind, true, 4, 4, 1, true, kLog>();
    if (vec4 && fast && d.CPL == 1) return compiled_compact_kernel<kKind, true, 0, 0, 1, true, kLog>();
    if (vec4 && fast) return compiled_compact_kernel<kKind, true, 0, 0, 0, true, kLog>();
    if (vec4) return compiled_compact_kernel<kKind, true, 0, 0, 0, false, kLog>();
    if (fast) return compiled_compact_kernel<kKind, false, 0, 0, 0, true, kLog>();
    return compiled_compact_kernel<kKind, false, 0, 0, 0, false, kLog>();
}

}  // namespace nastar

using namespace nastar;

extern "C" {

int nastar_version(void) { return NASTAR_VERSION; }

const char* nastar_last_error(void) { return g_last_error; }

size_t nastar_workspace_bytes(int B, int H, int W, int flags)
{
    if (B <= 0 || H <= 0 || W <= 0 || (long long)H * W > kMaxGlobalCells) return 0;
    return ws_layout(B, H, W, flags).total;  // 0: the whole search state lives in LDS and neither marks nor an order check were asked for
}

size_t nastar_batchloop_workspace_bytes(int B, int H, int W, int max_iters)
{
    if (B <= 0 || H <= 0 || W <= 0 || max_iters <= 0 || (long long)H * W > kMaxGlobalCells) return 0;
    return ws_layout(B, H, W, NASTAR_FLAG_MARK_COUPLED | NASTAR_FLAG_CHECK_ORDER).total + (size_t)B * (size_t)bitmap_words_for(max_iters) * 4;
}

// NASTAR_FLAG_CHECK_ORDER: one small launch that decides whether `order` is a permutation of 0..B-1; its verdict word is the LAST
// kOrderCheckBytes of the workspace and is read by the search / replay launch that follows on the same stream
static int check_order(const int32_t* order, int B, void* workspace, size_t workspace_bytes, size_t need, int32_t* summary, hipStream_t s,
                       const int** order_bad)
{
    // `need` = end of the verdict word inside the workspace (the word is the 16 bytes before it)
    *order_bad = nullptr;
    if (!workspace) return NASTAR_ERR_NULL;
    if (need < kOrderCheckBytes || workspace_bytes < need) return NASTAR_ERR_WORKSPACE;
    const size_t lds = (size_t)((B + 31) / 32) * 4;
    if (lds > kMaxLdsBytes - 64) return NASTAR_ERR_UNSUPPORTED;  // > 1.3 M maps in one launch: check the order on the caller's side
    int* bad = reinterpret_cast<int*>(static_cast<unsigned char*>(workspace) + need - kOrderCheckBytes);
    const int rc = launch_grid(nastar_order_check_kernel, dim3(1), dim3(1024), lds, s, order, B, bad, summary);
    if (rc == NASTAR_OK) *order_bad = bad;
    return rc;
}

// the lock-step launches of nastar_forward_batchloop_finish
struct LockArgs {
    const int* marks = nullptr;
    const int* t_end = nullptr;
    uint32_t* bitmap = nullptr;
    int bitmap_words = 0;
};

// one forward launch as an entry point describes it; the optional parts stay null (Moore-8) unless the entry point takes them
struct FwdLaunch {
    const float *cost, *start, *goal, *passable;
    int B, H, W;
    double g_ratio;
    int max_iters;
    float* histories_out;
    int64_t* paths_out;
    int32_t *sel_log_out, *iters_out, *status_out;
    void* workspace;
    size_t workspace_bytes;
    int flags;
    void* stream;
    uint8_t* packed_out = nullptr;
    const int32_t* order = nullptr;
    int32_t *order_out = nullptr, *summary = nullptr, *done_counter = nullptr;
    LockArgs lock = {};
    Neighbourhood nb = {};
    RouteOut route = {};  // routes_out, route_cap, route_len_out, route_cost_out of include/nastar_routes.h
    const int32_t* levels = nullptr;  // include/nastar_levels.h: the placement is ranked from these inside the launch (no order, no order_out)
    // include/nastar_ticket.h: the word the search launch stores ticket_value to when it starts, and where forward_lds says that the kernel
    // it launched carries the ticket (the first and the ranked compact kernel do; null for every other entry point)
    unsigned long long* ticket_word = nullptr;
    unsigned long long ticket_value = 0;
    bool* ticket_carried = nullptr;

    // the group nastar_forward_ex adds to nastar_forward, for it and the entry points that extend it
    void set_ex(uint8_t* packed, const int32_t* order_in, int32_t* order_o, int32_t* status_summary, int32_t* completion_counter)
    {
        packed_out = packed;
        order = order_in;
        order_out = order_o;
        summary = status_summary;
        done_counter = completion_counter;
    }
};

// does a launch of this shape have a kernel that ranks levels itself (nastar_forward_compact_ranked_kernel)?  Host only.  The hand-scheduled
// streams without a selection log: not the unit-cost layout, not lock-step mode, no compiled loop, no map outside LDS
static bool levels_in_launch(int H, int W, int flags, bool want_log)
{
    if (want_log || H != W || (W != 16 && W != 32 && W != 64)) return false;
    if (flags & ~kKnownFlags) return false;
    return (flags & (NASTAR_FLAG_UNIT_COST | NASTAR_FLAG_LOCKSTEP | NASTAR_FLAG_NO_ASM)) == 0;
}

// large map: cells in the caller's HBM workspace, open list in LDS (nastar_search_hybrid.hip.h)
static int forward_hybrid(const FwdLaunch& f, int* marks_out)
{
    if (!f.workspace) return NASTAR_ERR_NULL;
    const size_t slab = hybrid_slab_bytes(f.H * f.W);
    if (f.workspace_bytes < (size_t)f.B * slab) return NASTAR_ERR_WORKSPACE;
    hipStream_t s = reinterpret_cast<hipStream_t>(f.stream);
    FwdHybridArgs ha;
    ha.cost = f.cost; ha.start = f.start; ha.goal = f.goal; ha.passable = f.passable;
    ha.hist = f.histories_out; ha.paths = reinterpret_cast<long long*>(f.paths_out);
    ha.sel_log = f.sel_log_out; ha.iters = f.iters_out; ha.status = f.status_out; ha.summary = f.summary;
    ha.workspace = static_cast<unsigned char*>(f.workspace); ha.slab_bytes = slab; ha.max_iters = f.max_iters;
    ha.marks_out = marks_out;
    ha.marks = f.lock.marks; ha.t_end = f.lock.t_end; ha.bitmap = f.lock.bitmap; ha.bitmap_words = f.lock.bitmap_words;
    ha.route = f.route;
    HybridDims& hd = ha.d;
    hd.H = f.H; hd.W = f.W; hd.HW = f.H * f.W;
    hd.nchunks = (hd.HW + 63) / 64; hd.nsuper = (hd.nchunks + 63) / 64; hd.spl = (hd.nsuper + 63) / 64;
    hd.gr = (float)f.g_ratio; hd.omg = (float)(1.0 - f.g_ratio); hd.sqrtW = (float)sqrt((double)f.W);
    hd.rcp_sqrtW = 1.0f / hd.sqrtW;
    hd.inv_W = 1.0f / (float)f.W;
    // headers (start / goal cell per map) to -1: the fill launch raises them with atomicMax
    const unsigned per_map = (unsigned)((hd.nchunks * 64 + 255) / 256);
    const dim3 grid2(per_map < 64u ? per_map : 64u, (unsigned)f.B);
    const dim3 grid1((unsigned)((f.B + 255) / 256));
    int rc;
    if (f.nb.h0) {  // (the fill launch also looks at every heuristic value once: a NaN / infinite one marks its map in the header)
        rc = launch_grid(nastar_hybrid_header_heuristic_kernel, grid1, dim3(256), 0, s, ha.workspace, slab, hybrid_header_offset(hd.HW), f.B);
        if (rc == NASTAR_OK) rc = launch_grid(nastar_hybrid_fill_heuristic_kernel, grid2, dim3(256), 0, s, ha, f.nb.h0);
    } else {
        rc = launch_grid(nastar_hybrid_header_kernel, grid1, dim3(256), 0, s, ha.workspace, slab, hybrid_header_offset(hd.HW), f.B);
        if (rc == NASTAR_OK) rc = launch_grid(nastar_hybrid_fill_kernel, grid2, dim3(256), 0, s, ha);
    }
    if (rc) return rc;
    const size_t hl = hybrid_lds_bytes(hd.HW);
    if (hl > kMaxLdsBytes) return NASTAR_ERR_UNSUPPORTED;
    rc = f.nb.multi ? with_bools([&](auto fd, auto lk, auto heur) {
        return launch(nastar_forward_hybrid_sources_kernel<fd, lk, heur>, f.B, hl, s, ha, f.nb.mask, f.nb.h0);
    }, fastdiv_verified(f.W), (f.flags & NASTAR_FLAG_LOCKSTEP) != 0, f.nb.h0 != nullptr)
    : with_bools([&](auto fd, auto lk, auto masked, auto heur) {
        if constexpr (heur) return launch(nastar_forward_hybrid_heuristic_kernel<fd, lk>, f.B, hl, s, ha, f.nb.mask, f.nb.h0);
        else if constexpr (masked) return launch(nastar_forward_hybrid_masked_kernel<fd, lk>, f.B, hl, s, ha, f.nb.mask);
        else return launch(nastar_forward_hybrid_kernel<fd, lk>, f.B, hl, s, ha);
    }, fastdiv_verified(f.W), (f.flags & NASTAR_FLAG_LOCKSTEP) != 0, f.nb.masked, f.nb.h0 != nullptr);
    if (rc || ha.bitmap) return rc;  // (a probe launch has no outputs)
    return launch_grid(nastar_hybrid_store_kernel, grid2, dim3(256), 0, s, ha);
}

// unit-cost layout (nastar_search_unit.hip.h)
static int forward_unit(const FwdCArgs& c, int* marks_out, size_t lds, float rcp, hipStream_t s)
{
    if (marks_out) {  // unit costs are never in the batch-coupled class (f(n) - f(goal) >= 1.001 - 0.001 g_ratio > 0 with every cost 1)
        hipError_t me = hipMemsetAsync(marks_out, 0, (size_t)c.B * 4, s);
        if (me != hipSuccess) return hip_fail(me, "hipMemsetAsync");
    }
    if (c.d.W == 32) return launch(&nastar_forward_unit_kernel<5, false>, c.B, lds, s, c, rcp);
    if (c.flags & NASTAR_FLAG_NO_DIVE) return launch(&nastar_forward_unit_kernel<6, false>, c.B, lds, s, c, rcp);
    return launch(&nastar_forward_unit_kernel<6, true>, c.B, lds, s, c, rcp);
}

// maps whose state fits LDS: the unit-cost layout or the compact state (nastar_search_compact.hip.h)
static int forward_lds(const FwdLaunch& f, int* marks_out, bool& packed_done)
{
    FwdCArgs c;
    int rc = make_cdims(f.B, f.H, f.W, f.max_iters, f.g_ratio, c.d);
    if (rc) return rc;
    const size_t state_lds = f.nb.h0 ? compact_heur_lds_bytes(c.d.HWp, c.d.NCp) : compact_lds_bytes(c.d.HWp, c.d.NCp);
    if (state_lds > kMaxLdsBytes) return NASTAR_ERR_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(f.stream);
    c.cost = f.cost; c.start = f.start; c.goal = f.goal; c.passable = f.passable;
    c.hist = f.histories_out; c.paths = reinterpret_cast<long long*>(f.paths_out);
    c.sel_log = f.sel_log_out; c.iters = f.iters_out; c.status = f.status_out; c.max_iters = f.max_iters;
    c.packed = nullptr;
    c.order = f.order;
    c.order_out = f.order_out;  // (decided below: in-kernel completion order, or a rank of the step counts after the launch)
    c.summary = f.summary;
    c.done_counter = f.summary ? f.done_counter : nullptr;
    c.order_bad = nullptr;
    c.marks_out = marks_out;
    c.marks = f.lock.marks; c.t_end = f.lock.t_end; c.bitmap = f.lock.bitmap; c.bitmap_words = f.lock.bitmap_words;
    c.route = f.route;
    if (f.order && (f.flags & NASTAR_FLAG_CHECK_ORDER)) {
        rc = check_order(f.order, f.B, f.workspace, f.workspace_bytes, ws_layout(f.B, f.H, f.W, f.flags).chk_off + kOrderCheckBytes, f.summary, s,
                         &c.order_bad);
        if (rc) return rc;
    }
    c.flags = f.flags;
    c.B = f.B;
    const bool vec4 = (f.W % 4 == 0) && aligned16(f.cost) && aligned16(f.start) && aligned16(f.goal) && aligned16(f.passable) &&
                      aligned16(f.histories_out) && aligned16(f.paths_out) && aligned16(f.nb.h0);
    if (f.packed_out && vec4 && (c.d.HW % 8 == 0)) {  // fused emission of the bit-packed masks
        c.packed = f.packed_out;
        packed_done = true;
    }
    const float rcp = 1.0f / c.d.sqrtW;
    const bool fast = fastdiv_verified(f.W);
    // the hand-scheduled streams: Moore-8 only, and lock-step mode lives in the compiled step loops
    const bool use_asm = !f.nb.masked && !(f.flags & (NASTAR_FLAG_NO_ASM | NASTAR_FLAG_LOCKSTEP));
    // the launch's dynamic LDS: a hand-scheduled instantiation (Moore-8 kernel or the ranked one, built-in heuristic, one source) has guard rows
    const int kind = f.nb.multi ? (f.nb.h0 ? 4 : 3) : f.nb.h0 ? 2 : f.nb.masked ? 1 : 0;  // (compiled_compact_kernel's kKind)
    const bool asm_stream = takes_asm_stream(c.d, kind, vec4, fast, use_asm);
    const size_t lds = asm_stream ? compact_launch_lds_bytes(f.H, f.W, c.d.HWp, c.d.NCp, true) : state_lds;
    // unit-cost layout: the caller promises cost == passable with values in {0, 1} (checked per map by the kernel); taken when the promise can
    // hold at all (ONE tensor), no selection log is wanted and the hand-scheduled stream exists for the size
    const bool unit = (f.flags & NASTAR_FLAG_UNIT_COST) && f.cost == f.passable && use_asm && !(f.flags & (NASTAR_FLAG_ASM_V2 | NASTAR_FLAG_ASM_V3)) &&
                      !f.sel_log_out && vec4 && fast && f.g_ratio >= 0.0 && f.g_ratio <= 1.0 && f.H == f.W && (f.W == 32 || f.W == 64);
    const size_t kernel_lds = !unit ? lds : f.W == 32 ? (size_t)AsmLayoutUnit<5>::BYTES : (size_t)AsmLayoutUnit<6>::BYTES;
    // order_out: a launch whose maps are all resident at once ranks them by completion (one atomic per map, in the kernel); with several
    // rounds of workgroups completion time says when a map was STARTED, not how long its search was -- rank the step counts after the launch
    // (longest first; the trailing counter cell is not used and stays 0)
    const bool rank_after = f.order_out && (long long)f.B > resident_capacity(kernel_lds);
    if (rank_after) c.order_out = nullptr;
    unsigned long long* const tw = f.ticket_word;
    const unsigned long long tv = f.ticket_value;
    if (f.levels) {  // (nastar_forward_levels checked the shape, the flags and the log: what is left is the alignment of the caller's pointers)
        if (!asm_stream || unit) return NASTAR_ERR_UNSUPPORTED;  // (the ranked kernel exists as hand-scheduled instantiations only)
        const int* lv = f.levels;
        rc = f.W == 32   ? launch(&nastar_forward_compact_ranked_kernel<true, 5, 5, 1, true, false, true>, f.B, lds, s, c, rcp, lv, tw, tv)
             : f.W == 16 ? launch(&nastar_forward_compact_ranked_kernel<true, 4, 4, 1, true, false, true>, f.B, lds, s, c, rcp, lv, tw, tv)
                         : launch(&nastar_forward_compact_ranked_kernel<true, 6, 6, 4, true, false, true>, f.B, lds, s, c, rcp, lv, tw, tv);
        if (rc == NASTAR_OK && f.ticket_carried) *f.ticket_carried = true;  // (a launch that was accepted: only that one will store the ticket)
    } else
    if (unit) rc = forward_unit(c, marks_out, kernel_lds, rcp, s);
    else if (f.nb.multi) rc = with_bools([&](auto heur, auto lg) {  // (always masked: Moore-8 is a mask like any other here)
        return launch(compact_kernel<(heur ? 4 : 3), lg>(c.d, vec4, fast, false), f.B, lds, s, c, rcp, f.nb.mask, f.nb.h0);
    }, f.nb.h0 != nullptr, f.sel_log_out != nullptr);
    else rc = with_bools([&](auto masked, auto heur, auto lg) {
        const auto kern = compact_kernel<(heur ? 2 : masked ? 1 : 0), lg>(c.d, vec4, fast, asm_stream);
        if constexpr (heur) return launch(kern, f.B, lds, s, c, rcp, f.nb.mask, f.nb.h0);
        else if constexpr (masked) return launch(kern, f.B, lds, s, c, rcp, f.nb.mask);
        else {
            const int lrc = launch(kern, f.B, lds, s, c, rcp, tw, tv);
            if (lrc == NASTAR_OK && f.ticket_carried) *f.ticket_carried = true;
            return lrc;
        }
    }, f.nb.masked, f.nb.h0 != nullptr, f.sel_log_out != nullptr);
    return (rc == NASTAR_OK && rank_after) ? nastar_placement_from_levels(f.iters_out, f.B, f.order_out, f.stream) : rc;
}

// every forward entry point: the launch, then the bit-packed masks for shapes whose kernel does not emit them
static int forward(const FwdLaunch& f)
{
    if ((f.order || f.order_out) && f.B > 0 && f.H > 0 && f.W > 0 && needs_global_state(f.H, f.W)) return NASTAR_ERR_UNSUPPORTED;  // LDS-resident searches only
    if (!f.cost || !f.start || !f.goal || !f.passable || !f.histories_out || !f.paths_out || !f.iters_out || !f.status_out)
        return NASTAR_ERR_NULL;
    if (f.flags & ~kKnownFlags) return NASTAR_ERR_UNSUPPORTED;  // (A/B switches of the development build: make dev, csrc/nastar_dev_flags.h)
    if (f.B <= 0 || f.H <= 0 || f.W <= 0 || f.max_iters <= 0) return NASTAR_ERR_BAD_SHAPE;
    if ((long long)f.H * f.W > kMaxGlobalCells) return NASTAR_ERR_UNSUPPORTED;
    const WsLayout wl = ws_layout(f.B, f.H, f.W, f.flags);
    if (wl.total > 0) {
        if (!f.workspace) return NASTAR_ERR_NULL;
        if (f.workspace_bytes < wl.total) return NASTAR_ERR_WORKSPACE;
    }
    int* marks_out = (!(f.flags & NASTAR_FLAG_LOCKSTEP) && (f.flags & NASTAR_FLAG_MARK_COUPLED))
                         ? reinterpret_cast<int*>(static_cast<unsigned char*>(f.workspace) + wl.marks_off) : nullptr;
    bool packed_done = false;
    const int rc = needs_global_state(f.H, f.W) ? forward_hybrid(f, marks_out) : forward_lds(f, marks_out, packed_done);
    if (rc != NASTAR_OK || packed_done || !f.packed_out) return rc;
    return nastar_pack_outputs(f.histories_out, f.paths_out, f.B, f.H, f.W, f.packed_out, f.stream);
}

int nastar_forward(const float* cost, const float* start, const float* goal, const float* passable, int B, int H,
                   int W, double g_ratio, int max_iters, float* histories_out, int64_t* paths_out,
                   int32_t* sel_log_out, int32_t* iters_out, int32_t* status_out, void* workspace,
                   size_t workspace_bytes, int flags, void* stream)
{
    return forward(FwdLaunch{cost, start, goal, passable, B, H, W, g_ratio, max_iters, histories_out, paths_out, sel_log_out, iters_out,
                             status_out, workspace, workspace_bytes, flags, stream});
}

int nastar_forward_ordered(const float* cost, const float* start, const float* goal, const float* passable, int B, int H,
                           int W, double g_ratio, int max_iters, float* histories_out, int64_t* paths_out,
                           int32_t* sel_log_out, int32_t* iters_out, int32_t* status_out, uint8_t* packed_out, void* workspace,
                           size_t workspace_bytes, int flags, const int32_t* order, int32_t* order_out, void* stream)
{
    FwdLaunch f{cost, start, goal, passable, B, H, W, g_ratio, max_iters, histories_out, paths_out, sel_log_out, iters_out, status_out,
                workspace, workspace_bytes, flags, stream};
    f.packed_out = packed_out;
    f.order = order;
    f.order_out = order_out;
    return forward(f);
}

int nastar_forward_ex(const float* cost, const float* start, const float* goal, const float* passable, int B, int H, int W, double g_ratio,
                      int max_iters, float* histories_out, int64_t* paths_out, int32_t* sel_log_out, int32_t* iters_out, int32_t* status_out,
                      uint8_t* packed_out, void* workspace, size_t workspace_bytes, int flags, const int32_t* order, int32_t* order_out,
                      int32_t* status_summary, int32_t* completion_counter, void* stream)
{
    FwdLaunch f{cost, start, goal, passable, B, H, W, g_ratio, max_iters, histories_out, paths_out, sel_log_out, iters_out, status_out,
                workspace, workspace_bytes, flags, stream};
    f.set_ex(packed_out, order, order_out, status_summary, completion_counter);
    return forward(f);
}

int nastar_forward_ex_masked(const float* cost, const float* start, const float* goal, const float* passable, int B, int H, int W, double g_ratio,
                             int max_iters, float* histories_out, int64_t* paths_out, int32_t* sel_log_out, int32_t* iters_out, int32_t* status_out,
                             uint8_t* packed_out, void* workspace, size_t workspace_bytes, int flags, const int32_t* order, int32_t* order_out,
                             int32_t* status_summary, int32_t* completion_counter, unsigned neighbor_mask, void* stream)
{
    if (!neighbor_mask_valid(neighbor_mask)) return NASTAR_ERR_UNSUPPORTED;
    FwdLaunch f{cost, start, goal, passable, B, H, W, g_ratio, max_iters, histories_out, paths_out, sel_log_out, iters_out, status_out,
                workspace, workspace_bytes, flags, stream};
    f.set_ex(packed_out, order, order_out, status_summary, completion_counter);
    f.nb = Neighbourhood{true, neighbor_mask};
    return forward(f);
}

int nastar_forward_ex_heuristic(const float* cost, const float* start, const float* goal, const float* passable, int B, int H, int W, double g_ratio,
                                int max_iters, float* histories_out, int64_t* paths_out, int32_t* sel_log_out, int32_t* iters_out, int32_t* status_out,
                                uint8_t* packed_out, void* workspace, size_t workspace_bytes, int flags, const int32_t* order, int32_t* order_out,
                                int32_t* status_summary, int32_t* completion_counter, unsigned neighbor_mask, const float* h0, void* stream)
{
    if (!neighbor_mask_valid(neighbor_mask)) return NASTAR_ERR_UNSUPPORTED;
    if (!h0) return NASTAR_ERR_NULL;
    FwdLaunch f{cost, start, goal, passable, B, H, W, g_ratio, max_iters, histories_out, paths_out, sel_log_out, iters_out, status_out,
                workspace, workspace_bytes, flags, stream};
    f.set_ex(packed_out, order, order_out, status_summary, completion_counter);
    f.nb = Neighbourhood{true, neighbor_mask, h0};
    return forward(f);
}

static int batchloop_finish(const FwdLaunch& f)
{
    if (!f.cost || !f.start || !f.goal || !f.passable || !f.histories_out || !f.paths_out || !f.iters_out || !f.status_out || !f.workspace)
        return NASTAR_ERR_NULL;
    if (f.B <= 0 || f.H <= 0 || f.W <= 0 || f.max_iters <= 0) return NASTAR_ERR_BAD_SHAPE;
    if ((long long)f.H * f.W > kMaxGlobalCells) return NASTAR_ERR_UNSUPPORTED;
    if (f.workspace_bytes < nastar_batchloop_workspace_bytes(f.B, f.H, f.W, f.max_iters)) return NASTAR_ERR_WORKSPACE;
    const WsLayout wl = ws_layout(f.B, f.H, f.W, NASTAR_FLAG_MARK_COUPLED | NASTAR_FLAG_CHECK_ORDER);
    unsigned char* ws = static_cast<unsigned char*>(f.workspace);
    const int* marks = reinterpret_cast<const int*>(ws + wl.marks_off);
    int* tcell = reinterpret_cast<int*>(ws + wl.tcell_off);
    uint32_t* bitmap = reinterpret_cast<uint32_t*>(ws + wl.total);
    const int words = bitmap_words_for(f.max_iters);
    FwdLaunch run = f;  // (its workspace check cannot fail: the lock-step layout is the slabs alone)
    run.flags = NASTAR_FLAG_LOCKSTEP;
    // 1. PROBE: the marked maps in lock-step mode over the whole budget; which steps select the goal?  (no outputs)
    run.sel_log_out = nullptr;
    run.lock = LockArgs{marks, nullptr, bitmap, words};
    int rc = forward(run);
    if (rc) return rc;
    // 2. the first step at which EVERY map of the batch selects its goal
    // (the kernel's own __shared__ cells count against the 64 KiB a launch may own without a raised limit: longer budgets AND in global memory)
    const int lds_words = words < kTendMaxLdsWords ? words : kTendMaxLdsWords;
    rc = launch_grid(nastar_batchloop_tend_kernel, dim3(1), dim3(kTendThreads), (size_t)lds_words * 4, reinterpret_cast<hipStream_t>(f.stream),
                     f.iters_out, f.status_out, marks, bitmap, words, f.B, f.max_iters, tcell, lds_words);
    if (rc) return rc;
    // 3. FINAL: the marked maps again, for exactly t_end + 1 steps, with outputs (and their rows of the selection log)
    run.sel_log_out = f.sel_log_out;
    run.lock = LockArgs{marks, tcell, nullptr, words};
    return forward(run);
}

int nastar_forward_batchloop_finish(const float* cost, const float* start, const float* goal, const float* passable, int B, int H, int W,
                                    double g_ratio, int max_iters, float* histories_out, int64_t* paths_out, int32_t* sel_log_out,
                                    int32_t* iters_out, int32_t* status_out, void* workspace, size_t workspace_bytes, void* stream)
{
    return batchloop_finish(FwdLaunch{cost, start, goal, passable, B, H, W, g_ratio, max_iters, histories_out, paths_out, sel_log_out, iters_out,
                                      status_out, workspace, workspace_bytes, 0, stream});
}

int nastar_forward_batchloop_finish_masked(const float* cost, const float* start, const float* goal, const float* passable, int B, int H, int W,
                                           double g_ratio, int max_iters, float* histories_out, int64_t* paths_out, int32_t* sel_log_out,
                                           int32_t* iters_out, int32_t* status_out, void* workspace, size_t workspace_bytes,
                                           unsigned neighbor_mask, void* stream)
{
    if (!neighbor_mask_valid(neighbor_mask)) return NASTAR_ERR_UNSUPPORTED;
    FwdLaunch f{cost, start, goal, passable, B, H, W, g_ratio, max_iters, histories_out, paths_out, sel_log_out, iters_out, status_out,
                workspace, workspace_bytes, 0, stream};
    f.nb = Neighbourhood{true, neighbor_mask};
    return batchloop_finish(f);
}

int nastar_forward_batchloop_finish_heuristic(const float* cost, const float* start, const float* goal, const float* passable, int B, int H, int W,
                                              double g_ratio, int max_iters, float* histories_out, int64_t* paths_out, int32_t* sel_log_out,
                                              int32_t* iters_out, int32_t* status_out, void* workspace, size_t workspace_bytes,
                                              unsigned neighbor_mask, const float* h0, void* stream)
{
    if (!neighbor_mask_valid(neighbor_mask)) return NASTAR_ERR_UNSUPPORTED;
    if (!h0) return NASTAR_ERR_NULL;
    FwdLaunch f{cost, start, goal, passable, B, H, W, g_ratio, max_iters, histories_out, paths_out, sel_log_out, iters_out, status_out,
                workspace, workspace_bytes, 0, stream};
    f.nb = Neighbourhood{true, neighbor_mask, h0};
    return batchloop_finish(f);
}

// ---- include/nastar_routes.h: the search launch that also returns every map's ordered route, its length and its cost ----------------------
int nastar_routes_abi(void) { return NASTAR_ROUTES_ABI; }

// the route group of both entry points, checked before any HIP call; the neighbourhood: Moore-8 without a heuristic is the launch of
// nastar_forward_ex (its kernels: hand-scheduled streams, unit-cost layout), any other mask the masked twins, a heuristic the third ones
static int routes_launch(FwdLaunch& f, unsigned neighbor_mask, const float* h0, int32_t* routes_out, int route_cap, int32_t* route_len_out,
                         float* route_cost_out)
{
    if (!neighbor_mask_valid(neighbor_mask)) return NASTAR_ERR_UNSUPPORTED;
    if (!routes_out || !route_len_out) return NASTAR_ERR_NULL;
    if (route_cap < 1) return NASTAR_ERR_BAD_SHAPE;
    if (h0) f.nb = Neighbourhood{true, neighbor_mask, h0};
    else if (neighbor_mask != NASTAR_NEIGHBORS_MOORE8) f.nb = Neighbourhood{true, neighbor_mask};
    f.route = RouteOut{routes_out, route_cap, route_len_out, route_cost_out};
    return NASTAR_OK;
}

int nastar_forward_routes(const float* cost, const float* start, const float* goal, const float* passable, int B, int H, int W, double g_ratio,
                          int max_iters, float* histories_out, int64_t* paths_out, int32_t* sel_log_out, int32_t* iters_out, int32_t* status_out,
                          uint8_t* packed_out, void* workspace, size_t workspace_bytes, int flags, const int32_t* order, int32_t* order_out,
                          int32_t* status_summary, int32_t* completion_counter, unsigned neighbor_mask, const float* h0, int32_t* routes_out,
                          int route_cap, int32_t* route_len_out, float* route_cost_out, void* stream)
{
    FwdLaunch f{cost, start, goal, passable, B, H, W, g_ratio, max_iters, histories_out, paths_out, sel_log_out, iters_out, status_out,
                workspace, workspace_bytes, flags, stream};
    const int rc = routes_launch(f, neighbor_mask, h0, routes_out, route_cap, route_len_out, route_cost_out);
    if (rc) return rc;
    f.set_ex(packed_out, order, order_out, status_summary, completion_counter);
    return forward(f);
}

int nastar_forward_routes_batchloop_finish(const float* cost, const float* start, const float* goal, const float* passable, int B, int H, int W,
                                           double g_ratio, int max_iters, float* histories_out, int64_t* paths_out, int32_t* sel_log_out,
                                           int32_t* iters_out, int32_t* status_out, void* workspace, size_t workspace_bytes,
                                           unsigned neighbor_mask, const float* h0, int32_t* routes_out, int route_cap, int32_t* route_len_out,
                                           float* route_cost_out, void* stream)
{
    FwdLaunch f{cost, start, goal, passable, B, H, W, g_ratio, max_iters, histories_out, paths_out, sel_log_out, iters_out, status_out,
                workspace, workspace_bytes, 0, stream};
    const int rc = routes_launch(f, neighbor_mask, h0, routes_out, route_cap, route_len_out, route_cost_out);
    if (rc) return rc;
    return batchloop_finish(f);  // (its FINAL launch rewrites the rows of the maps it re-runs: routes, lengths and costs with them)
}

// ---- include/nastar_sources.h: the search from EVERY non-zero cell of the start map, and its replay -----------------------------------------
int nastar_sources_abi(void) { return NASTAR_SOURCES_ABI; }

// the mask, the heuristic and the optional route group of both search entry points, checked before any HIP call.  A multi-source launch
// always runs the masked twins (Moore-8 is a mask like any other): the hand-scheduled streams and the unit-cost layout take no start set.
static int sources_launch(FwdLaunch& f, unsigned neighbor_mask, const float* h0, int32_t* routes_out, int route_cap, int32_t* route_len_out,
                          float* route_cost_out)
{
    if (!neighbor_mask_valid(neighbor_mask)) return NASTAR_ERR_UNSUPPORTED;
    if (routes_out) {
        if (!route_len_out) return NASTAR_ERR_NULL;
        if (route_cap < 1) return NASTAR_ERR_BAD_SHAPE;
        f.route = RouteOut{routes_out, route_cap, route_len_out, route_cost_out};
    }
    f.nb = Neighbourhood{true, neighbor_mask, h0, true};
    return NASTAR_OK;
}

int nastar_forward_sources(const float* cost, const float* start, const float* goal, const float* passable, int B, int H, int W, double g_ratio,
                           int max_iters, float* histories_out, int64_t* paths_out, int32_t* sel_log_out, int32_t* iters_out, int32_t* status_out,
                           uint8_t* packed_out, void* workspace, size_t workspace_bytes, int flags, const int32_t* order, int32_t* order_out,
                           int32_t* status_summary, int32_t* completion_counter, unsigned neighbor_mask, const float* h0, int32_t* routes_out,
                           int route_cap, int32_t* route_len_out, float* route_cost_out, void* stream)
{
    FwdLaunch f{cost, start, goal, passable, B, H, W, g_ratio, max_iters, histories_out, paths_out, sel_log_out, iters_out, status_out,
                workspace, workspace_bytes, flags, stream};
    const int rc = sources_launch(f, neighbor_mask, h0, routes_out, route_cap, route_len_out, route_cost_out);
    if (rc) return rc;
    f.set_ex(packed_out, order, order_out, status_summary, completion_counter);
    return forward(f);
}

int nastar_forward_sources_batchloop_finish(const float* cost, const float* start, const float* goal, const float* passable, int B, int H, int W,
                                            double g_ratio, int max_iters, float* histories_out, int64_t* paths_out, int32_t* sel_log_out,
                                            int32_t* iters_out, int32_t* status_out, void* workspace, size_t workspace_bytes,
                                            unsigned neighbor_mask, const float* h0, int32_t* routes_out, int route_cap, int32_t* route_len_out,
                                            float* route_cost_out, void* stream)
{
    FwdLaunch f{cost, start, goal, passable, B, H, W, g_ratio, max_iters, histories_out, paths_out, sel_log_out, iters_out, status_out,
                workspace, workspace_bytes, 0, stream};
    const int rc = sources_launch(f, neighbor_mask, h0, routes_out, route_cap, route_len_out, route_cost_out);
    if (rc) return rc;
    return batchloop_finish(f);  // (the PROBE and FINAL launches seed every start too: FwdLaunch::nb travels with them)
}

// ---- include/nastar_levels.h: the search launch that places its maps by their levels itself ------------------------------------------------
int nastar_levels_abi(void) { return NASTAR_LEVELS_ABI; }

int nastar_levels_in_launch(int H, int W, int flags, int want_log) { return levels_in_launch(H, W, flags, want_log != 0) ? 1 : 0; }

int nastar_forward_levels(const float* cost, const float* start, const float* goal, const float* passable, int B, int H, int W, double g_ratio,
                          int max_iters, float* histories_out, int64_t* paths_out, int32_t* sel_log_out, int32_t* iters_out, int32_t* status_out,
                          uint8_t* packed_out, void* workspace, size_t workspace_bytes, int flags, const int32_t* levels,
                          int32_t* status_summary, int32_t* completion_counter, void* stream)
{
    if (!levels) return NASTAR_ERR_NULL;
    if (!levels_in_launch(H, W, flags, sel_log_out != nullptr)) return NASTAR_ERR_UNSUPPORTED;
    FwdLaunch f{cost, start, goal, passable, B, H, W, g_ratio, max_iters, histories_out, paths_out, sel_log_out, iters_out, status_out,
                workspace, workspace_bytes, flags, stream};
    f.packed_out = packed_out;
    f.summary = status_summary;
    f.done_counter = completion_counter;
    f.levels = levels;
    return forward(f);
}

int nastar_placement_slots(const int32_t* levels, int B, int32_t* order_out, void* stream)
{
    if (!levels || !order_out) return NASTAR_ERR_NULL;
    if (B <= 0) return NASTAR_ERR_BAD_SHAPE;
    return launch(nastar_placement_slots_kernel, B, 0, reinterpret_cast<hipStream_t>(stream), levels, B, order_out);
}

int nastar_completion_supported(int H, int W)
{
    return (H > 0 && W > 0 && (long long)H * W <= kMaxGlobalCells && !needs_global_state(H, W)) ? 1 : 0;
}

int nastar_host_wait_nonzero(const volatile int32_t* word_host, int timeout_us)
{
    if (!word_host) return 0;
    timespec t0;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (unsigned spin = 0;; ++spin) {
        if (*word_host != 0) return 1;
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#elif defined(__aarch64__)
        asm volatile("yield");
#endif
        if ((spin & 255u) == 255u) {
            timespec t1;
            clock_gettime(CLOCK_MONOTONIC, &t1);
            const long long us = (long long)(t1.tv_sec - t0.tv_sec) * 1000000ll + (t1.tv_nsec - t0.tv_nsec) / 1000;
            if (us >= timeout_us) return *word_host != 0 ? 1 : 0;
        }
    }
}

int nastar_placement_from_levels(const int32_t* levels, int B, int32_t* order_out, void* stream)
{
    if (!levels || !order_out) return NASTAR_ERR_NULL;
    if (B <= 0) return NASTAR_ERR_BAD_SHAPE;
    return launch_grid(nastar_rank_levels_kernel, dim3(1), dim3(PLC_RANK_THREADS), 0, reinterpret_cast<hipStream_t>(stream), levels, B, order_out);
}

int nastar_placement_predict(const float* passable, const float* start, const float* goal, int B, int H, int W, int32_t* order_out,
                             void* workspace, size_t workspace_bytes, void* stream)
{
    if (!passable || !start || !goal || !order_out || !workspace) return NASTAR_ERR_NULL;
    if (B <= 0 || H <= 0 || W <= 0) return NASTAR_ERR_BAD_SHAPE;
    if (H != W || (W != 32 && W != 64) || !aligned16(passable) || !aligned16(start) || !aligned16(goal)) return NASTAR_ERR_UNSUPPORTED;
    if (workspace_bytes < (size_t)B * sizeof(int)) return NASTAR_ERR_WORKSPACE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int* level = static_cast<int*>(workspace);
    const int rc = W == 32 ? launch(nastar_bfs_level_kernel<5>, B, 0, s, passable, start, goal, B, level)
                           : launch(nastar_bfs_level_kernel<6>, B, 0, s, passable, start, goal, B, level);
    if (rc) return rc;
    return launch_grid(nastar_rank_levels_kernel, dim3(1), dim3(PLC_RANK_THREADS), 0, s, level, B, order_out);
}

int nastar_forward_packed(const float* cost, const float* start, const float* goal, const float* passable, int B, int H,
                          int W, double g_ratio, int max_iters, float* histories_out, int64_t* paths_out,
                          int32_t* sel_log_out, int32_t* iters_out, int32_t* status_out, uint8_t* packed_out,
                          void* workspace, size_t workspace_bytes, int flags, void* stream)
{
    if (!packed_out) return NASTAR_ERR_NULL;
    FwdLaunch f{cost, start, goal, passable, B, H, W, g_ratio, max_iters, histories_out, paths_out, sel_log_out, iters_out, status_out,
                workspace, workspace_bytes, flags, stream};
    f.packed_out = packed_out;
    return forward(f);
}

// ---- backward by replay of the forward's selection log (nastar_backward_replay.hip.h) ------------------------------------
// history entries per map: one per executed step.  An early-exit search executes at most HW + 1 selections whatever the budget; in LOCK-STEP mode
// a goal selection does not close a cell, but between two of them a map of the batch-coupled class closes at least one, and once it closes none it
// selects its goal at every step (the loop then ends as soon as every map does): at most 2 HW steps.  (Square maps: max_iters = W W = HW either way.)
static int bwdr_hist_len(int HW, int max_iters) { return (max_iters < 2 * HW + 2 ? max_iters : 2 * HW + 2) + 2; }
static bool bwdr_fits_lds(int HW) { return bwdr_state_bytes(((HW + 63) / 64) * 64) <= kMaxLdsBytes; }

// 32-bit history stamps (2 B more per cell of the HBM state): maps above 65,519 cells, or a history that can outrun 16 bits
static bool bwdr_wide(int HW, int max_iters) { return HW > 65535 - CCSZ || bwdr_hist_len(HW, max_iters) > 65535; }

size_t nastar_backward_workspace_bytes(int B, int H, int W, int max_iters)
{
    if (B <= 0 || H <= 0 || W <= 0 || max_iters <= 0 || (long long)H * W > kMaxGlobalCells) return 0;
    const int HW = H * W, HWp = ((HW + 63) / 64) * 64;
    size_t n = (size_t)B * (size_t)bwdr_hist_len(HW, max_iters) * 16;
    // (a wide history on an LDS-sized map -- a lock-step log beyond 65535 entries -- takes the HBM state too)
    const bool wide = bwdr_wide(HW, max_iters);
    if (wide || !bwdr_fits_lds(HW)) n += (size_t)B * ((bwdr_state_bytes(HWp, wide) + 255) & ~(size_t)255);
    return n + kOrderCheckBytes;  // + the verdict word of NASTAR_FLAG_CHECK_ORDER (nastar_backward_replay_ordered)
}

static int backward_replay_impl(BwdRArgs& a, const float* cost, const float* start, const float* goal, const float* passable,
                                const int32_t* sel_log, int B, int H, int W, double g_ratio, int max_iters, const int32_t* iters,
                                const int32_t* t_batch_dev, float* grad_cost_out, void* workspace, size_t workspace_bytes, void* stream,
                                int flags, Neighbourhood nb)
{
    if (!cost || !start || !goal || !passable || !sel_log || !iters || !grad_cost_out || !workspace) return NASTAR_ERR_NULL;
    if (B <= 0 || H <= 0 || W <= 0 || max_iters <= 0) return NASTAR_ERR_BAD_SHAPE;
    if ((long long)H * W > kMaxGlobalCells) return NASTAR_ERR_UNSUPPORTED;
    if ((long long)H * W > 65535 - CCSZ) {
        // above the compact layouts' 16-bit cell indices: the replay needs the geometry and the priority's constants only
        a.d = CompactDims{};
        a.d.H = H; a.d.W = W; a.d.HW = H * W;
        a.d.gr = (float)g_ratio;
        a.d.omg = (float)(1.0 - g_ratio);
        a.d.sqrtW = (float)sqrt((double)W);
    } else {
        int rc = make_cdims(B, H, W, max_iters, g_ratio, a.d);
        if (rc) return rc;
    }
    if (workspace_bytes < nastar_backward_workspace_bytes(B, H, W, max_iters)) return NASTAR_ERR_WORKSPACE;
    a.d.HWp = ((a.d.HW + 63) / 64) * 64;
    a.cost = cost; a.start = start; a.goal = goal; a.passable = passable; a.sel_log = sel_log; a.iters = iters;
    a.B_total = B;
    a.t_batch = t_batch_dev; a.grad_cost = grad_cost_out; a.max_iters = max_iters;
    a.kfac = a.d.omg * (-1.0f / a.d.sqrtW);
    a.hist = static_cast<double*>(workspace);
    // the kernel indexes the history by step: a search executes at most HW + 1 selections whatever the budget
    const int hlen = bwdr_hist_len(a.d.HW, max_iters);
    a.state = nullptr;
    a.state_stride = 0;
    a.hist_len = hlen;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const float rcp = 1.0f / a.d.sqrtW;
    const bool fast = fastdiv_verified(W);
    const int max_steps = hlen - 2;
    if ((flags & ~(kKnownFlags)) != 0) return NASTAR_ERR_UNSUPPORTED;
    const bool wide = bwdr_wide(a.d.HW, max_iters);  // (history stamps are 16-bit otherwise)
    // (the hand-scheduled loop closes every selected cell: a lock-step log, whose goal selections leave the goal open, takes the general loop)
    if (!nb.masked && (flags & (NASTAR_FLAG_NO_ASM | NASTAR_FLAG_LOCKSTEP)) == 0 && fast && H == W && (W == 32 || W == 16) && aligned16(cost) && aligned16(start) &&
        aligned16(goal) && aligned16(passable) && aligned16(grad_cost_out) && bwdr_asm_lds_bytes(a.d.HW, max_steps) <= kMaxLdsBytes) {
        // hand-scheduled replay loop (nastar_backward_replay_asm.hip.h): the reference's training sizes
        const size_t lds = bwdr_asm_lds_bytes(a.d.HW, max_steps);
        return W == 32 ? launch(nastar_backward_replay_asm_kernel<5>, B, lds, s, a, rcp)
                       : launch(nastar_backward_replay_asm_kernel<4>, B, lds, s, a, rcp);
    }
    if (!wide && bwdr_fits_lds(a.d.HW)) {
        // history in LDS as long as at least 2 maps (or what the state alone allows) stay resident per CU
        const size_t st = bwdr_state_bytes(a.d.HWp), with_hist = st + (size_t)hlen * 16;
        const bool hist_lds = with_hist <= kMaxLdsBytes && (kMaxLdsBytes / with_hist >= 2 || kMaxLdsBytes / st < 2);
        if (nb.multi) return with_bools([&](auto hl, auto fd, auto heur) {
            return launch(nastar_backward_replay_sources_kernel<false, hl, fd, heur>, B, hl ? with_hist : st, s, a, rcp, nb.mask, nb.h0);
        }, hist_lds, fast, nb.h0 != nullptr);
        return with_bools([&](auto hl, auto fd, auto masked, auto heur) {
            const size_t lds = hl ? with_hist : st;
            if constexpr (heur) return launch(nastar_backward_replay_heuristic_kernel<false, hl, fd>, B, lds, s, a, rcp, nb.mask, nb.h0);
            else if constexpr (masked) return launch(nastar_backward_replay_masked_kernel<false, hl, fd>, B, lds, s, a, rcp, nb.mask);
            else return launch(nastar_backward_replay_kernel<false, hl, fd>, B, lds, s, a, rcp);
        }, hist_lds, fast, nb.masked, nb.h0 != nullptr);
    }
    // state in the HBM workspace: FILL (all CUs: slab, zeroed gradient, start / goal cells into the slab's header), REPLAY (one wavefront per map:
    // O(steps)), SWEEP (all CUs: the cells still open at the end) -- nastar_backward_replay.hip.h
    a.state_stride = (bwdr_state_bytes(a.d.HWp, wide) + 255) & ~(size_t)255;
    a.state = static_cast<unsigned char*>(workspace) + (size_t)B * (size_t)hlen * 16;
    // headers (start / goal cell per map) to -1: the fill launch raises them with atomicMax (the forward's header kernel: same layout of two ints)
    int rc = launch_grid(nastar_hybrid_header_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, a.state, a.state_stride,
                         bwdr_header_offset(a.d.HWp, wide), B);
    if (rc) return rc;
    const unsigned per_map = (unsigned)((a.d.HW + 255) / 256);
    const dim3 grid2(per_map < 64u ? per_map : 64u, (unsigned)B);
    rc = with_bools([&](auto w) { return launch_grid(nastar_bwdr_fill_kernel<w>, grid2, dim3(256), 0, s, a); }, wide);
    if (rc) return rc;
    rc = nb.multi ? with_bools([&](auto fd, auto w, auto heur) {
        return launch(nastar_backward_replay_sources_kernel<true, false, fd, heur, w>, B, 64, s, a, rcp, nb.mask, nb.h0);
    }, fast, wide, nb.h0 != nullptr)
    : with_bools([&](auto fd, auto w, auto masked, auto heur) {
        if constexpr (heur) return launch(nastar_backward_replay_heuristic_kernel<true, false, fd, w>, B, 64, s, a, rcp, nb.mask, nb.h0);
        else if constexpr (masked) return launch(nastar_backward_replay_masked_kernel<true, false, fd, w>, B, 64, s, a, rcp, nb.mask);
        else return launch(nastar_backward_replay_kernel<true, false, fd, w>, B, 64, s, a, rcp);
    }, fast, wide, nb.masked, nb.h0 != nullptr);
    if (rc != NASTAR_OK) return rc;
    return with_bools([&](auto w, auto fd, auto heur) {
        if constexpr (heur) return launch_grid(nastar_bwdr_sweep_heuristic_kernel<w, fd>, grid2, dim3(256), 0, s, a, rcp, nb.h0);
        else return launch_grid(nastar_bwdr_sweep_kernel<w, fd>, grid2, dim3(256), 0, s, a, rcp);
    }, wide, fast, nb.h0 != nullptr);
}

int nastar_backward_replay(const float* grad_histories, const float* cost, const float* start, const float* goal,
                           const float* passable, const int32_t* sel_log, int B, int H, int W, double g_ratio, int max_iters,
                           const int32_t* iters, const int32_t* t_batch_dev, float* grad_cost_out, void* workspace,
                           size_t workspace_bytes, int flags, void* stream)
{
    if (!grad_histories) return NASTAR_ERR_NULL;
    BwdRArgs a;
    a.grad_hist = grad_histories; a.l1_hist = nullptr; a.l1_traj = nullptr; a.l1_up = nullptr; a.l1_scale = 0.f;
    a.order = nullptr;
    a.order_bad = nullptr;
    return backward_replay_impl(a, cost, start, goal, passable, sel_log, B, H, W, g_ratio, max_iters, iters, t_batch_dev,
                                grad_cost_out, workspace, workspace_bytes, stream, flags, Neighbourhood{});
}

int nastar_backward_l1_replay(const float* histories, const float* opt_trajs, const float* grad_loss_dev, const float* cost,
                              const float* start, const float* goal, const float* passable, const int32_t* sel_log, int B, int H,
                              int W, double g_ratio, int max_iters, const int32_t* iters, const int32_t* t_batch_dev,
                              float* grad_cost_out, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!histories || !opt_trajs) return NASTAR_ERR_NULL;
    if (B <= 0 || H <= 0 || W <= 0) return NASTAR_ERR_BAD_SHAPE;
    BwdRArgs a;
    a.grad_hist = nullptr; a.l1_hist = histories; a.l1_traj = opt_trajs; a.l1_up = grad_loss_dev;
    a.l1_scale = (float)(1.0 / ((double)B * H * W));
    a.order = nullptr;
    a.order_bad = nullptr;
    return backward_replay_impl(a, cost, start, goal, passable, sel_log, B, H, W, g_ratio, max_iters, iters, t_batch_dev,
                                grad_cost_out, workspace, workspace_bytes, stream, 0, Neighbourhood{});
}

static int backward_replay_ordered_impl(const float* grad_histories, const float* histories, const float* opt_trajs, const float* grad_loss_dev,
                                        const float* cost, const float* start, const float* goal, const float* passable, const int32_t* sel_log,
                                        int B, int H, int W, double g_ratio, int max_iters, const int32_t* iters, const int32_t* t_batch_dev,
                                        float* grad_cost_out, void* workspace, size_t workspace_bytes, int flags, const int32_t* order,
                                        Neighbourhood nb, void* stream)
{
    if (!grad_histories && (!histories || !opt_trajs)) return NASTAR_ERR_NULL;
    if (B <= 0 || H <= 0 || W <= 0) return NASTAR_ERR_BAD_SHAPE;
    BwdRArgs a;
    a.grad_hist = grad_histories;
    a.l1_hist = grad_histories ? nullptr : histories; a.l1_traj = grad_histories ? nullptr : opt_trajs;
    a.l1_up = grad_histories ? nullptr : grad_loss_dev;
    a.l1_scale = grad_histories ? 0.f : (float)(1.0 / ((double)B * H * W));
    a.order = order;
    a.order_bad = nullptr;
    if (order && (flags & NASTAR_FLAG_CHECK_ORDER)) {
        // the verdict word sits behind the replay's own workspace (nastar_backward_workspace_bytes already includes it)
        const size_t need = nastar_backward_workspace_bytes(B, H, W, max_iters);
        if (need == 0) return NASTAR_ERR_UNSUPPORTED;
        int rc = check_order(order, B, workspace, workspace_bytes, need, nullptr, reinterpret_cast<hipStream_t>(stream), &a.order_bad);
        if (rc) return rc;
    }
    return backward_replay_impl(a, cost, start, goal, passable, sel_log, B, H, W, g_ratio, max_iters, iters, t_batch_dev,
                                grad_cost_out, workspace, workspace_bytes, stream, flags, nb);
}

int nastar_backward_replay_ordered(const float* grad_histories, const float* histories, const float* opt_trajs, const float* grad_loss_dev,
                                   const float* cost, const float* start, const float* goal, const float* passable, const int32_t* sel_log,
                                   int B, int H, int W, double g_ratio, int max_iters, const int32_t* iters, const int32_t* t_batch_dev,
                                   float* grad_cost_out, void* workspace, size_t workspace_bytes, int flags, const int32_t* order, void* stream)
{
    return backward_replay_ordered_impl(grad_histories, histories, opt_trajs, grad_loss_dev, cost, start, goal, passable, sel_log, B, H, W, g_ratio,
                                        max_iters, iters, t_batch_dev, grad_cost_out, workspace, workspace_bytes, flags, order,
                                        Neighbourhood{}, stream);
}

int nastar_backward_replay_ordered_masked(const float* grad_histories, const float* histories, const float* opt_trajs, const float* grad_loss_dev,
                                          const float* cost, const float* start, const float* goal, const float* passable, const int32_t* sel_log,
                                          int B, int H, int W, double g_ratio, int max_iters, const int32_t* iters, const int32_t* t_batch_dev,
                                          float* grad_cost_out, void* workspace, size_t workspace_bytes, int flags, const int32_t* order,
                                          unsigned neighbor_mask, void* stream)
{
    if (!neighbor_mask_valid(neighbor_mask)) return NASTAR_ERR_UNSUPPORTED;
    return backward_replay_ordered_impl(grad_histories, histories, opt_trajs, grad_loss_dev, cost, start, goal, passable, sel_log, B, H, W, g_ratio,
                                        max_iters, iters, t_batch_dev, grad_cost_out, workspace, workspace_bytes, flags, order,
                                        Neighbourhood{true, neighbor_mask}, stream);
}

int nastar_backward_replay_ordered_heuristic(const float* grad_histories, const float* histories, const float* opt_trajs, const float* grad_loss_dev,
                                             const float* cost, const float* start, const float* goal, const float* passable, const int32_t* sel_log,
                                             int B, int H, int W, double g_ratio, int max_iters, const int32_t* iters, const int32_t* t_batch_dev,
                                             float* grad_cost_out, void* workspace, size_t workspace_bytes, int flags, const int32_t* order,
                                             unsigned neighbor_mask, const float* h0, void* stream)
{
    if (!neighbor_mask_valid(neighbor_mask)) return NASTAR_ERR_UNSUPPORTED;
    if (!h0) return NASTAR_ERR_NULL;
    return backward_replay_ordered_impl(grad_histories, histories, opt_trajs, grad_loss_dev, cost, start, goal, passable, sel_log, B, H, W, g_ratio,
                                        max_iters, iters, t_batch_dev, grad_cost_out, workspace, workspace_bytes, flags, order,
                                        Neighbourhood{true, neighbor_mask, h0}, stream);
}

int nastar_backward_replay_sources(const float* grad_histories, const float* histories, const float* opt_trajs, const float* grad_loss_dev,
                                   const float* cost, const float* start, const float* goal, const float* passable, const int32_t* sel_log,
                                   int B, int H, int W, double g_ratio, int max_iters, const int32_t* iters, const int32_t* t_batch_dev,
                                   float* grad_cost_out, void* workspace, size_t workspace_bytes, int flags, const int32_t* order,
                                   unsigned neighbor_mask, const float* h0, void* stream)
{
    if (!neighbor_mask_valid(neighbor_mask)) return NASTAR_ERR_UNSUPPORTED;
    return backward_replay_ordered_impl(grad_histories, histories, opt_trajs, grad_loss_dev, cost, start, goal, passable, sel_log, B, H, W, g_ratio,
                                        max_iters, iters, t_batch_dev, grad_cost_out, workspace, workspace_bytes, flags, order,
                                        Neighbourhood{true, neighbor_mask, h0, true}, stream);
}

// workgroups of the pack / unpack kernels: 256 lanes, one per packed byte of a plane, grid-stride beyond 8192 workgroups
static unsigned pack_grid(int B, int nb)
{
    const long long total = (long long)B * nb;
    return (unsigned)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
}

int nastar_pack_outputs(const float* histories, const int64_t* paths, int B, int H, int W, uint8_t* packed_out, void* stream)
{
    if (!histories || !paths || !packed_out) return NASTAR_ERR_NULL;
    if (B <= 0 || H <= 0 || W <= 0) return NASTAR_ERR_BAD_SHAPE;
    const int HW = H * W, nb = (HW + 7) / 8;
    return launch_grid(nastar_pack_kernel, dim3(pack_grid(B, nb)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), histories,
                       reinterpret_cast<const long long*>(paths), packed_out, B, HW, nb);
}

int nastar_unpack_outputs(const uint8_t* packed, int B, int H, int W, float* histories_out, int64_t* paths_out, void* stream)
{
    if (!histories_out || !paths_out || !packed) return NASTAR_ERR_NULL;
    if (B <= 0 || H <= 0 || W <= 0) return NASTAR_ERR_BAD_SHAPE;
    const int HW = H * W, nb = (HW + 7) / 8;
    return launch_grid(nastar_unpack_kernel, dim3(pack_grid(B, nb)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), packed,
                       histories_out, reinterpret_cast<long long*>(paths_out), B, HW, nb);
}

int nastar_debug_occupancy(int H, int W, int* lds_bytes_out)
{
    CompactDims d;
    if (make_cdims(1, H, W, 1, 0.5, d)) return -1;
    // the kernel and the size of a default launch: the hand-scheduled instantiation with its guard rows where one exists
    const size_t lds = compact_launch_lds_bytes(H, W, d.HWp, d.NCp, true);
    if (lds_bytes_out) *lds_bytes_out = (int)lds;
    if (lds > kMaxLdsBytes) return 0;
    void (*kern)(const FwdCArgs, const float, unsigned long long*, const unsigned long long) = &nastar_forward_compact_kernel<true, 0, 0, 0, false, false>;
    if (H == 16 && W == 16) kern = &nastar_forward_compact_kernel<true, 4, 4, 1, true, false, true>;
    if (H == 32 && W == 32) kern = &nastar_forward_compact_kernel<true, 5, 5, 1, true, false, true>;
    if (H == 64 && W == 64) kern = &nastar_forward_compact_kernel<true, 6, 6, 4, true, false, true>;
    if (ensure_lds(kern, lds)) return -1;
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, 64, lds) != hipSuccess) return -1;
    return nb;
}

int nastar_heuristic(const float* goal, int B, int H, int W, float* h0_out, void* stream)
{
    if (!goal || !h0_out) return NASTAR_ERR_NULL;
    if (B <= 0 || H <= 0 || W <= 0) return NASTAR_ERR_BAD_SHAPE;
    if ((long long)H * W > kMaxGlobalCells) return NASTAR_ERR_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if ((long long)H * W > 65535) return launch_grid(nastar_heuristic_large_kernel, dim3((unsigned)B), dim3(256), 0, s, goal, h0_out, H, W);
    const uint32_t magicW = (uint32_t)((1ull << 32) / (unsigned)W) + 1u;
    return launch(nastar_heuristic_kernel, B, 0, s, goal, h0_out, H, W, magicW);
}

}  // extern "C"

// ---- csrc/nastar_ticket.hip.h: the search launch of include/nastar_ticket.h (its entry point is in nastar_verdict_capi.hip) -----------------
bool nastar::search_carries_ticket(int H, int W, int flags)
{
    return H > 0 && W > 0 && (long long)H * W <= kMaxGlobalCells && !needs_global_state(H, W) && !(flags & NASTAR_FLAG_UNIT_COST);
}

int nastar::forward_ticketed(const TicketedSearch& t, bool* carried)
{
    *carried = false;
    if (t.levels && !levels_in_launch(t.H, t.W, t.flags, t.sel_log_out != nullptr)) return NASTAR_ERR_UNSUPPORTED;  // (as nastar_forward_levels)
    FwdLaunch f{t.cost, t.start, t.goal, t.passable, t.B, t.H, t.W, t.g_ratio, t.max_iters, t.histories_out, t.paths_out, t.sel_log_out, t.iters_out,
                t.status_out, t.workspace, t.workspace_bytes, t.flags, t.stream};
    if (t.levels) f.set_ex(t.packed_out, nullptr, nullptr, t.status_summary, t.completion_counter);
    else f.set_ex(t.packed_out, t.order, t.order_out, t.status_summary, t.completion_counter);
    f.levels = t.levels;
    f.ticket_word = t.ticket_word;
    f.ticket_value = t.ticket_value;
    f.ticket_carried = carried;
    return forward(f);
}
