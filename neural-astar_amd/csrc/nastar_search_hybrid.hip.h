// nastar_search_hybrid.hip.h -- forward search for maps too large for LDS (129x129 ... 1024x1024: as long as the open list's chunk minima fit
// the 160 KiB of one CU, 8 B per 64 cells): the OPEN LIST lives in LDS, the cells in HBM.
//
// The reference's answer to large maps is "use the CPU pq_astar" (astar.py:36-37) because its loop touches every cell of every map
// per step (differentiable_astar.py:203-252).  Here a step touches 64 + 8 + 1 cells.  State of one map (one 64-lane wavefront):
//
//   HBM slab (5 B/cell, caller's workspace; L2-resident in practice)
//     g[]     fp32, the node state in the sign of infinity exactly as in the LDS kernels (nastar_search.hip.h): +inf passable & never
//             opened, -inf closed or obstacle, finite = open.  "relax neighbour n" (:229,:235) is the one comparison g[n] > g2.
//     pdir[]  parent direction | passable | on-path bits (1 B)
//     cost is NOT copied: it is read from the caller's tensor when a cell is touched; h0 is recomputed from the coordinates.
//   LDS (8 B per 64 cells + 512 B: 33 KB at 512x512, 130 KB at 1024x1024)
//     cmin[c] per 64-cell chunk: (key << 32 | cell) of its first minimal open cell, ~0 when it holds none   (u64 order = first-index tie-break)
//     smin[s] per 64 chunks: the minimum of their cmin entries
//
// Three launches per call (fill / search / store, see below).  A step of the search (round 4's kernel kept all three levels in HBM and paid
// SEVEN dependent L2 round trips per step; round 5's read the open list back from LDS twice per step and ran five wave minima in series):
//   select   nothing to do: (key, cell) of s* is in two scalar registers, left there by the previous step
//   load     g / cost of s*, of its 8 neighbours and of the 64 cells of its chunk: issued together, ONE round trip               (HBM)
//   shadow   while that round trip is in flight: the open list WITHOUT s* 's chunk and super-chunk -- restS = minimum of the other 63 chunk
//            entries of its super-chunk, restE = minimum of the other super-chunk entries (two wave minima side by side, LDS reads issued
//            before the loads) -- and both heuristics (the chunk's cells, the neighbours)
//   update   newC = the chunk's minimum without s*, nbr = minimum of the relaxed neighbours (one 64-lane and one 8-lane minimum side by
//            side); g / pdir stores; cmin[C] = newC and smin[S] = min(restS, newC) by plain writes, the neighbours enter both levels by
//            ds_min_u64 -- nothing is read back                                                                                     (LDS)
//   next     s* of the next step = min(restE, restS, newC, nbr): every open cell is in exactly one of the four sets          (scalar)
// All four are first-index minima of (key << 32 | cell): entries ascend with the lane in each set, so "the first lane holding the minimal
// key" (ballot + s_ff1 + v_readlane) replaces a second wave minimum over the cells.
// Keys are never stored: q = fl(f / fl32(sqrt(W))) is re-derived from (g, cost, coordinates), with the IEEE division (no reciprocal).
#pragma once
#include "nastar_search.hip.h"
#include "nastar_routes.hip.h"

namespace nastar {

struct HybridDims {
    int H, W, HW;
    int nchunks;   // ceil(HW / 64)
    int nsuper;    // ceil(nchunks / 64)
    int spl;       // super-chunk entries per lane = ceil(nsuper / 64): 1 up to 512x512, 4 at 1024x1024 (lane l owns entries [l spl, (l + 1) spl))
    float gr, omg, sqrtW, rcp_sqrtW;
    float inv_W;   // 1 / W: row of a flat index by one multiply + one correction step (see hybrid_row)
};

// per map: g[HWp] fp32 | pdir[HWp] u8 | (256-byte aligned) header {start cell, goal cell} written by the fill kernel
__host__ __device__ inline size_t hybrid_header_offset(int HW)
{
    const size_t HWp = (((size_t)HW + 63) / 64) * 64;
    return (HWp * 5 + 255) & ~(size_t)255;
}
__host__ __device__ inline size_t hybrid_slab_bytes(int HW) { return hybrid_header_offset(HW) + 256; }
// cmin: one entry per chunk, padded to whole super-chunks; smin: one entry per super-chunk, padded to `spl` entries for each of the 64 lanes
__host__ __device__ inline size_t hybrid_lds_bytes(int HW)
{
    const size_t nchunks = ((size_t)HW + 63) / 64;
    const size_t nsuper = (nchunks + 63) / 64;
    const size_t spl = (nsuper + 63) / 64;
    return nsuper * 64 * 8 + spl * 64 * 8;
}

struct FwdHybridArgs {
    const float* cost;
    const float* start;
    const float* goal;
    const float* passable;
    float* hist;
    long long* paths;
    int* sel_log;
    int* iters;
    int* status;
    int* summary;
    unsigned char* workspace;
    size_t slab_bytes;
    int max_iters;
    int* marks_out;        // early-exit launch, optional [B]: 1 = this map reached its goal but is not at a fixed point of the reference's batch loop
    const int* marks;      // lock-step launches, optional [B]: search only the maps marked 1
    const int* t_end;      // lock-step FINAL launch, optional device cell: the budget is *t_end + 1 steps
    uint32_t* bitmap;      // lock-step PROBE launch: [B][bitmap_words], bit t = the goal was selected at step t
    int bitmap_words;
    HybridDims d;
    RouteOut route;        // optional (include/nastar_routes.h): ordered routes, lengths, costs; null for every entry point of nastar.h
};

// row of flat index i (< 2^21, rows up to 393215 on a 393216x3 map): the product is within (r + 1) 2^-23 of (i + 0.5) / W, which lies 0.5 / W
// from an integer -- already the row while H W < 2^22; the one correction step either way is a margin no accepted map uses
__device__ __forceinline__ int hybrid_row(int i, const HybridDims& d, int& c)
{
    int r = (int)(((float)i + 0.5f) * d.inv_W);
    c = i - r * d.W;
    if (c < 0) { --r; c += d.W; }
    else if (c >= d.W) { ++r; c -= d.W; }
    return r;
}

// the same without branches (selects): the if / else-if form above compiles to two divergent regions, i.e. two VALU -> SALU -> VALU hops
__device__ __forceinline__ int hybrid_row_nb(int i, const HybridDims& d, int& c)
{
    const int r0 = (int)(((float)i + 0.5f) * d.inv_W);
    const int c0 = i - r0 * d.W;
    const bool lo = c0 < 0, hi = c0 >= d.W;
    c = lo ? c0 + d.W : (hi ? c0 - d.W : c0);
    return lo ? r0 - 1 : (hi ? r0 + 1 : r0);
}

// first-index minimum of per-lane (key, cell) entries = the u64 minimum of (key << 32 | cell), in every lane and without leaving the vector
// registers: the key minimum, then the cell minimum among the lanes that hold it.  (A scalar form -- v_readlane of the minimum, ballot, s_ff1,
// v_readlane of the cell -- is three instructions shorter and was 28 % SLOWER per step: each VALU -> SALU -> VALU hop costs a lone wavefront
// ~25 cycles, profiles/r05/probe_large_scalar_reductions.jsonl.)
__device__ __forceinline__ unsigned long long first_min_entry(uint32_t key, uint32_t cell)
{
    const uint32_t m = wave_min_all_u32(key);
    const uint32_t c = wave_min_all_u32(key == m ? cell : 0xFFFFFFFFu);
    return m == KEY_INF ? ~0ull : (((unsigned long long)m << 32) | c);
}

template <bool kFastDiv>
__device__ __forceinline__ uint32_t hybrid_key(const HybridDims& d, float g, float h)
{
    const float f = d.gr * g + d.omg * h;   // :206  f = g_ratio * g + (1 - g_ratio) * h
    float q;
    if constexpr (kFastDiv) {
        // correctly rounded f / sqrt(W) (exhaustively verified per W, tools/fastdiv_check.c; the LDS kernels use the same three instructions)
        const float q0 = f * d.rcp_sqrtW;
        const float rem = __builtin_fmaf(-q0, d.sqrtW, f);
        q = __builtin_fmaf(rem, d.rcp_sqrtW, q0);
    } else {
        q = f / d.sqrtW;                    // :207  the quotient the reference's softmax orders by (IEEE division)
    }
    return f32_to_ord(q);
}

// Three launches on the caller's stream: FILL (all CUs: node states from the passable map, start / goal cells into the slab header), SEARCH
// (one wavefront per map: as many maps resident per CU as wave slots allow -- a step is an L2 round trip, residency is what hides it), STORE
// (all CUs: histories / paths from the slab).  One wavefront filling and storing 262144 cells took 5 ms per map.
__global__ __launch_bounds__(256) void nastar_hybrid_fill_kernel(const FwdHybridArgs a)
{
    const int b = blockIdx.y;
    if (a.marks != nullptr && a.marks[b] == 0) return;  // lock-step launches touch only the marked maps
    const HybridDims d = a.d;
    const int HWp = d.nchunks * 64;
    unsigned char* const slab = a.workspace + (size_t)b * a.slab_bytes;
    float* const g = reinterpret_cast<float*>(slab);
    uint8_t* const pdir = reinterpret_cast<uint8_t*>(g + HWp);
    int* const hdr = reinterpret_cast<int*>(slab + hybrid_header_offset(d.HW));  // {-1, -1} on entry (hipMemsetAsync 0xFF)
    const size_t off = (size_t)b * (size_t)d.HW;
    int sidx = -1, gidx = -1;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HWp; i += gridDim.x * 256) {
        const bool valid = i < d.HW;
        if (valid && a.start[off + i] != 0.f) sidx = i;
        if (valid && a.goal[off + i] != 0.f) gidx = i;
        const bool pass = valid && a.passable[off + i] != 0.f;
        g[i] = pass ? NASTAR_POS_INF : NASTAR_NEG_INF;
        pdir[i] = (uint8_t)(PARENT_UNSET | (pass ? P_PASS : 0u));
    }
    if (sidx >= 0) atomicMax(&hdr[0], sidx);  // (the LAST non-zero cell, like the LDS kernels)
    if (gidx >= 0) atomicMax(&hdr[1], gidx);
}

__global__ __launch_bounds__(256) void nastar_hybrid_header_kernel(unsigned char* workspace, size_t slab_bytes, size_t header_off, int B)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B) {  // (also for maps a lock-step launch skips: their headers are not read again)
        int* hdr = reinterpret_cast<int*>(workspace + (size_t)b * slab_bytes + header_off);
        hdr[0] = -1;
        hdr[1] = -1;
    }
}

__global__ __launch_bounds__(256) void nastar_hybrid_store_kernel(const FwdHybridArgs a)
{
    const int b = blockIdx.y;
    if (a.marks != nullptr && a.marks[b] == 0) return;
    const HybridDims d = a.d;
    const int HWp = d.nchunks * 64;
    const unsigned char* const slab = a.workspace + (size_t)b * a.slab_bytes;
    const float* const g = reinterpret_cast<const float*>(slab);
    const uint8_t* const pdir = reinterpret_cast<const uint8_t*>(g + HWp);
    const size_t off = (size_t)b * (size_t)d.HW;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < d.HW; i += gridDim.x * 256) {
        const uint32_t m = pdir[i];
        a.hist[off + i] = ((m & P_PASS) && g[i] == NASTAR_NEG_INF) ? 1.0f : 0.0f;  // closed list (:222-223)
        a.paths[off + i] = (m & P_PATH) ? 1 : 0;
    }
    if (a.route.routes != nullptr) {  // the -1 tail of the map's route row (the search launch wrote the cells and the length)
        const int len = a.route.len[b];
        int* const row = a.route.routes + (size_t)b * (size_t)a.route.cap;
        for (int i = (len < a.route.cap ? len : a.route.cap) + blockIdx.x * 256 + threadIdx.x; i < a.route.cap; i += gridDim.x * 256) row[i] = -1;
    }
}

// How the search reaches its slab -- decided by measurement in round 5 (profiles/r05/probe_large_variants_*.jsonl; the A/B switches lived in
// the library until round 6):
//   * plain accesses through the CU's vector L1 instead of agent-scope (sc1) ones served by L2 (986 instead of 1275 ns per step).  The slab of a
//     map is touched by ONE wavefront between the fill and the store launch, and the lanes of a wavefront are coherent through their L1 without
//     further action (it is write-through and processes a wavefront's accesses in order): the neighbourhood of s* is mostly the neighbourhood
//     of the previous one, i.e. L1 hits.
//   * s* travels in a SCALAR register (v_readlane of the reduction's result): the loop's exits (open list empty, goal selected, budget) are
//     scalar branches and the step counter a scalar -- the compiler otherwise treats the wave-uniform s* as divergent and wraps every exit in
//     exec-mask bookkeeping; rows / columns by selects instead of branches (hybrid_row_nb): -7 %.
//   * the selection's tie-break by ballot + first set lane + v_readlane instead of a second wave minimum (entries ascend with the lane): -1 %.
//   * the wait for the previous step's stores before this step's loads stays (dropping it changed nothing: 938-940 ns).
//
// kLock: the LOCK-STEP modes (the reference's batch loop to the letter, differentiable_astar.py:219-225, :251): a selected goal is expanded
// like any cell and stays on the open list, and the map is stepped on -- PROBE (a.bitmap != nullptr: no outputs; bit t of the map's bitmap
// row = "the goal was selected at step t", over the whole budget) and FINAL (outputs after exactly *a.t_end + 1 steps).  With a.marks only
// the maps the early-exit launch marked as batch-coupled are searched; the others return at once (their outputs stand).
__device__ __forceinline__ float hld(const float* p) { return *p; }
__device__ __forceinline__ uint32_t hld(const uint8_t* p) { return *p; }

// does the expansion of the goal cell s (selected just now) open or lower a neighbour that BEATS the goal?  (wave-uniform; lanes 0..7)
template <bool kFastDiv>
__device__ __forceinline__ bool hybrid_goal_beaten(const HybridDims& d, const float* g, const float* cost, int s, int lane, int dr, int dc,
                                                   int goal_r, int goal_c)
{
    int gc0;
    const int gr0 = hybrid_row_nb(s, d, gc0);
    const int nr = gr0 + dr, nc = gc0 + dc;
    const bool inb = (lane < 8) & ((unsigned)nr < (unsigned)d.H) & ((unsigned)nc < (unsigned)d.W);
    const int n = inb ? s + dr * d.W + dc : s;
    global_step_fence();
    const float gs = g[s], gn = g[n];
    const float cs = cost[s], cn = cost[n];
    const float g2 = gs + cs;
    const uint32_t kn = hybrid_key<kFastDiv>(d, g2, heuristic0(nr, nc, goal_r, goal_c) + cn);
    const uint32_t kg = hybrid_key<kFastDiv>(d, gs, heuristic0(gr0, gc0, goal_r, goal_c) + cs);
    const bool beats = inb & (gn > g2) & ((kn < kg) | ((kn == kg) & (n < s)));
    return __ballot(beats) != 0ull;
}

// the same test in the masked kernel: `nb` = this lane relaxes its neighbour (lanes 0-7 that the neighbor_filter opens, neighbour_enabled)
template <bool kFastDiv>
__device__ __forceinline__ bool hybrid_goal_beaten_gated(const HybridDims& d, const float* g, const float* cost, int s, bool nb, int dr, int dc,
                                                         int goal_r, int goal_c)
{
    int gc0;
    const int gr0 = hybrid_row_nb(s, d, gc0);
    const int nr = gr0 + dr, nc = gc0 + dc;
    const bool inb = nb & ((unsigned)nr < (unsigned)d.H) & ((unsigned)nc < (unsigned)d.W);
    const int n = inb ? s + dr * d.W + dc : s;
    global_step_fence();
    const float gs = g[s], gn = g[n];
    const float cs = cost[s], cn = cost[n];
    const float g2 = gs + cs;
    const uint32_t kn = hybrid_key<kFastDiv>(d, g2, heuristic0(nr, nc, goal_r, goal_c) + cn);
    const uint32_t kg = hybrid_key<kFastDiv>(d, gs, heuristic0(gr0, gc0, goal_r, goal_c) + cs);
    const bool beats = inb & (gn > g2) & ((kn < kg) | ((kn == kg) & (n < s)));
    return __ballot(beats) != 0ull;
}

// the same test with a caller-supplied heuristic: h0 of the neighbour and of the goal itself are loaded (h0(goal) need not be 0)
template <bool kFastDiv>
__device__ __forceinline__ bool hybrid_goal_beaten_heuristic(const HybridDims& d, const float* g, const float* cost, const float* h0m, int s,
                                                             bool nb, int dr, int dc)
{
    int gc0;
    const int gr0 = hybrid_row_nb(s, d, gc0);
    const int nr = gr0 + dr, nc = gc0 + dc;
    const bool inb = nb & ((unsigned)nr < (unsigned)d.H) & ((unsigned)nc < (unsigned)d.W);
    const int n = inb ? s + dr * d.W + dc : s;
    global_step_fence();
    const float gs = g[s], gn = g[n];
    const float cs = cost[s], cn = cost[n];
    const float hs = h0m[s], hn = h0m[n];
    const float g2 = gs + cs;
    const uint32_t kn = hybrid_key<kFastDiv>(d, g2, hn + cn);
    const uint32_t kg = hybrid_key<kFastDiv>(d, gs, hs + cs);
    const bool beats = inb & (gn > g2) & ((kn < kg) | ((kn == kg) & (n < s)));
    return __ballot(beats) != 0ull;
}

// the fill launch of a search with a caller-supplied heuristic: nastar_hybrid_fill_kernel, and every h0 value of the map is looked at
// once -- hdr[2] (0 on entry: nastar_hybrid_header_heuristic_kernel) becomes 1 when one is NaN or infinite (NASTAR_ERR_BAD_HEURISTIC)
__global__ __launch_bounds__(256) void nastar_hybrid_fill_heuristic_kernel(const FwdHybridArgs a, const float* __restrict__ h0)
{
    const int b = blockIdx.y;
    if (a.marks != nullptr && a.marks[b] == 0) return;  // lock-step launches touch only the marked maps
    const HybridDims d = a.d;
    const int HWp = d.nchunks * 64;
    unsigned char* const slab = a.workspace + (size_t)b * a.slab_bytes;
    float* const g = reinterpret_cast<float*>(slab);
    uint8_t* const pdir = reinterpret_cast<uint8_t*>(g + HWp);
    int* const hdr = reinterpret_cast<int*>(slab + hybrid_header_offset(d.HW));
    const size_t off = (size_t)b * (size_t)d.HW;
    int sidx = -1, gidx = -1;
    bool bad = false;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HWp; i += gridDim.x * 256) {
        const bool valid = i < d.HW;
        if (valid && a.start[off + i] != 0.f) sidx = i;
        if (valid && a.goal[off + i] != 0.f) gidx = i;
        if (valid) bad |= !(fabsf(h0[off + i]) < NASTAR_POS_INF);
        const bool pass = valid && a.passable[off + i] != 0.f;
        g[i] = pass ? NASTAR_POS_INF : NASTAR_NEG_INF;
        pdir[i] = (uint8_t)(PARENT_UNSET | (pass ? P_PASS : 0u));
    }
    if (sidx >= 0) atomicMax(&hdr[0], sidx);
    if (gidx >= 0) atomicMax(&hdr[1], gidx);
    if (bad) atomicMax(&hdr[2], 1);
}

__global__ __launch_bounds__(256) void nastar_hybrid_header_heuristic_kernel(unsigned char* workspace, size_t slab_bytes, size_t header_off, int B)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B) {
        int* hdr = reinterpret_cast<int*>(workspace + (size_t)b * slab_bytes + header_off);
        hdr[0] = -1;
        hdr[1] = -1;
        hdr[2] = 0;
    }
}

// The seeding pass of the multi-source kernels (nastar_forward_hybrid_sources_kernel), run by the searching wavefront before its first step:
// every non-zero cell of `start` is opened with g = 0 and an unset parent (on an obstacle too) and enters cmin / smin by ds_min_u64 on
// (key << 32 | cell), so that several starts in one chunk or super-chunk leave the first minimal one behind.  The start map is read 16 cells
// per lane and trip (four 16-byte loads in flight) where its row is 16-byte aligned.  Returns the first selection, the minimum over smin
// (wave-uniform; ~0 = no source).  The fill launch cannot do this: the open list lives in the LDS of the searching wavefront, and the
// built-in heuristic needs the goal cell, which the fill launch is still looking for.
template <bool kFastDiv, bool kHeur>
__device__ __forceinline__ unsigned long long hybrid_open_sources(const HybridDims& d, float* g, uint8_t* pdir, unsigned long long* cmin,
                                                                  unsigned long long* smin, const float* cost, const float* h0m,
                                                                  const float* __restrict__ start, int lane, int goal_r, int goal_c)
{
    auto open = [&](int i) {
        float h;
        if constexpr (kHeur) {
            h = h0m[i] + cost[i];
        } else {
            int c;
            const int r = hybrid_row_nb(i, d, c);
            h = heuristic0(r, c, goal_r, goal_c) + cost[i];  // :191-192 h = h0 + cost
        }
        const unsigned long long e = ((unsigned long long)hybrid_key<kFastDiv>(d, 0.0f, h) << 32) | (uint32_t)i;
        g[i] = 0.0f;
        pdir[i] = (uint8_t)(PARENT_UNSET | P_PASS);
        atomicMin(&cmin[i >> 6], e);
        atomicMin(&smin[i >> 12], e);
    };
    int done = 0;
    if ((d.HW & 3) == 0 && (reinterpret_cast<uintptr_t>(start) & 15u) == 0) {
        const float4* s4 = reinterpret_cast<const float4*>(start);
        const int n4 = d.HW >> 2;
        int q = lane;
        for (; q + 192 < n4; q += 256) {
            float4 sv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) sv[k] = s4[q + 64 * k];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = (q + 64 * k) << 2;
                if (sv[k].x != 0.f) open(i);
                if (sv[k].y != 0.f) open(i + 1);
                if (sv[k].z != 0.f) open(i + 2);
                if (sv[k].w != 0.f) open(i + 3);
            }
        }
        for (; q < n4; q += 64) {
            const float4 sv = s4[q];
            const int i = q << 2;
            if (sv.x != 0.f) open(i);
            if (sv.y != 0.f) open(i + 1);
            if (sv.z != 0.f) open(i + 2);
            if (sv.w != 0.f) open(i + 3);
        }
        done = d.HW;
    }
    for (int i = done + lane; i < d.HW; i += 64)
        if (start[i] != 0.f) open(i);
    global_step_fence();
    __syncthreads();
    // the first selection: the u64 minimum over the super-chunk entries (lane l owns [l spl, (l + 1) spl), ascending cells)
    unsigned long long e0 = smin[lane * d.spl];
    for (int j = 1; j < d.spl; ++j) {
        const unsigned long long ej = smin[lane * d.spl + j];
        e0 = ej < e0 ? ej : e0;
    }
    const unsigned long long m = first_min_entry((uint32_t)(e0 >> 32), (uint32_t)e0);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)m), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(m >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

// kMasked: the neighbourhood of DifferentiableAstar.neighbor_filter (nmask, see neighbour_enabled) instead of the Moore-8 stencil.
// kHeur (nastar_forward_hybrid_heuristic_kernel): h0 is the caller's tensor instead of the built-in heuristic; it always takes the mask.
// All three kernels share one body, nastar_forward_hybrid_body.inc.
template <bool kFastDiv, bool kLock = false>
__global__ __launch_bounds__(64) void nastar_forward_hybrid_kernel(const FwdHybridArgs a)
{
    constexpr bool kMasked = false, kHeur = false, kMulti = false;
    constexpr uint32_t nmask = 0x1EFu;  // (NASTAR_NEIGHBORS_MOORE8; never read)
    constexpr const float* h0 = nullptr;
#include "nastar_forward_hybrid_body.inc"
}

template <bool kFastDiv, bool kLock>
__global__ __launch_bounds__(64) void nastar_forward_hybrid_masked_kernel(const FwdHybridArgs a, const uint32_t nmask)
{
    constexpr bool kMasked = true, kHeur = false, kMulti = false;
    constexpr const float* h0 = nullptr;
#include "nastar_forward_hybrid_body.inc"
}

template <bool kFastDiv, bool kLock>
__global__ __launch_bounds__(64) void nastar_forward_hybrid_heuristic_kernel(const FwdHybridArgs a, const uint32_t nmask, const float* __restrict__ h0)
{
    constexpr bool kMasked = true, kHeur = true, kMulti = false;
#include "nastar_forward_hybrid_body.inc"
}

// the MULTI-SOURCE search (include/nastar_sources.h): kHeur = false, the masked kernel's step with the built-in heuristic (h0 is not read);
// kHeur = true, the heuristic kernel's.  Both take the neighbourhood mask.
template <bool kFastDiv, bool kLock, bool kHeur>
__global__ __launch_bounds__(64) void nastar_forward_hybrid_sources_kernel(const FwdHybridArgs a, const uint32_t nmask, const float* __restrict__ h0)
{
    constexpr bool kMasked = true, kMulti = true;
#include "nastar_forward_hybrid_body.inc"
}

}  // namespace nastar
