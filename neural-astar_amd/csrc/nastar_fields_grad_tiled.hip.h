// nastar_fields_grad_tiled.hip.h -- the gradient of the cost-to-go field with respect to the cost maps for maps too large for one workgroup:
// the subtree sum of include/nastar_fields_grad.h, tiled (include/nastar_fields_grad_tiled.h).
//
// Definition, rounding rule and summation order are those of item 6g, written once in nastar_field_rules.hip.h (fld_best_action,
// fld_child_set, fld_subtree_sum, fld_sweep); the geometry is that of item 6f (nastar_tile_geometry.hip.h): tiles of kTileH x kTileW
// cells, one 256-lane workgroup per (map, tile), two alternating flag arrays, per-map words.  The workspace holds, per cell, the fp64
// accumulator A (8 B) and one successor byte.  Three kernels:
//   init    per cell: live or not, and the successor (fld_best_action on the readable field, one-cell halo read from HBM); writes the
//           successor byte, A = G on live cells and 0 elsewhere, raises the map's plateau word for a live cell without a successor, marks
//           the tile active when it holds a live cell;
//   round   a tile that is not active, or whose map has the plateau word, exits.  An active one loads A and the successor bytes, interior
//           plus a one-cell halo ("no child" outside the map), into LDS; a lane keeps G and the 8-bit child set of its 16 cells in
//           registers; fld_sweep recomputes IN PLACE every cell that has a child (fld_subtree_sum) to the LOCAL fixed point (halo fixed;
//           bounded by the tile's cell count); then it stores the interior cells whose bits differ from what HBM holds and ends the round
//           with tld_end_round on the adjacent tile that holds the successor of such a cell (the only tile that reads it);
//   finish  grad_cost = fl32(A) on live cells, 0.0f elsewhere; all zeros for a map with a plateau or an active tile left; the status.
// Inside a launch nothing is handed from one workgroup to another.  A cell is a pure function of its children's values and the forest has
// no cycle: there is ONE fixed point, and a tile that read a stale halo word has been marked by its writer, so a state with no tile marked
// IS that fixed point, whatever raced past on the way (the values are not monotone: the argument is uniqueness, not bounds).  A words in
// HBM are read and written through relaxed agent-scope 64-bit atomics (vector accesses; an 8-byte word is never torn), flags and per-map
// words through tld_load / tld_store.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nastar_fields_grad_tiled.h"
#include "nastar_fields_grad.hip.h"
#include "nastar_tile_geometry.hip.h"

namespace nastar {

constexpr int kGradTiledMaxCells = kTiledMaxCells;
constexpr uint8_t kNoSucc = 0xFF;  // not live, or live without a successor (a plateau)

struct GradTiledArgs {
    const float* dist;       // [B,HW]
    const float* goal;
    const float* passable;
    const float* grad_dist;  // [B,HW], or nullptr: the plateau verdict alone (init writes no A)
    float* grad_cost;        // [B,HW]
    int32_t* status;         // [B]
    int32_t* visits;         // [B] or nullptr
    double* acc;             // [B,HW]: A
    uint8_t* succ;           // [B,HW]
    int32_t* words;          // [4,B]: the last round in which the map marked a tile, the last round in which it relaxed one, plateau, unused
    int32_t* flags;          // [2,B*tiles]
    TileGrid g;
    uint32_t nmask;
};

__device__ __forceinline__ double gtl_load(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void gtl_store(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(kTileT) void nastar_fields_grad_tiled_init_kernel(const GradTiledArgs a)
{
    const TilePos p = tld_pos(a.g);
    const int tid = threadIdx.x, H = a.g.H, W = a.g.W;
    const float* dist = a.dist + p.base;
    const float* goal = a.goal + p.base;
    const float* pass = a.passable + p.base;
    const uint32_t nm = a.nmask;
    const float INF = INFINITY;
    bool any_live = false, stuck = false;
    const int cc = tid & (kTileW - 1);
    if (cc < p.cols) {
        const int x = p.x0 + cc;
        for (int rr = tid / kTileW; rr < p.rows; rr += kTileT / kTileW) {
            const int y = p.y0 + rr;
            const ptrdiff_t i = (ptrdiff_t)y * W + x;
            const float d = dist[i];
            const bool live = goal[i] == 0.f && d < INF;  // (a NaN is not below +inf: not live)
            int best = -1;
            if (live) {
                auto readable = [&](int dy, int dx) {
                    const ptrdiff_t j = i + (ptrdiff_t)dy * W + dx;
                    return pass[j] != 0.f ? dist[j] : INF;
                };
                best = fld_best_action(readable, nm, y > 0, y < H - 1, x > 0, x < W - 1, d);
                stuck |= best < 0;
                any_live = true;
            }
            a.succ[p.base + (size_t)i] = best < 0 ? kNoSucc : (uint8_t)best;
            if (a.grad_dist) gtl_store(a.acc + p.base + (size_t)i, live ? (double)a.grad_dist[p.base + (size_t)i] : 0.0);
        }
    }
    const int tile_live = __syncthreads_or(any_live), tile_stuck = __syncthreads_or(stuck);
    if (tid == 0) {
        const size_t nflags = (size_t)a.g.B * a.g.ty * a.g.tx;
        tld_store(a.flags + blockIdx.x, tile_live ? 1 : 0);
        tld_store(a.flags + nflags + blockIdx.x, 0);
        if (tile_stuck) tld_store(a.words + 2 * (size_t)a.g.B + p.b, 1);
        if (p.t == 0 && a.visits) a.visits[p.b] = 0;
    }
}

// the plateau verdict alone: behind an init launch
__global__ __launch_bounds__(kTileT) void nastar_fields_grad_tiled_status_kernel(const GradTiledArgs a)
{
    const size_t b = (size_t)blockIdx.x * kTileT + threadIdx.x;
    if (b < (size_t)a.g.B) a.status[b] = tld_load(a.words + 2 * (size_t)a.g.B + b) != 0 ? NASTAR_ERR_PLATEAU : NASTAR_OK;
}

// round: 1, 2, ... ; the flags of round r are array (r - 1) & 1
__global__ __launch_bounds__(kTileT) void nastar_fields_grad_tiled_round_kernel(const GradTiledArgs a, const int round)
{
    __shared__ double A[kHaloH * kHaloW];           // interior + halo; the halo is never written
    __shared__ uint8_t S[kHaloH * kHaloW + 4];      // the successor bytes of the same cells
    __shared__ int flags[8];                        // [0..2] sweep flags, [3] the adjacent tiles that read a cell this one changed
    constexpr int K = kGradCellsPerLane;
    constexpr int kRowStep = kTileT / kTileW;
    const size_t nflags = (size_t)a.g.B * a.g.ty * a.g.tx;
    int32_t* cur = a.flags + (size_t)((round - 1) & 1) * nflags;
    int32_t* nxt = a.flags + (size_t)(round & 1) * nflags;
    const TilePos p = tld_pos(a.g);
    // 1. not active this round, or a map with a plateau: nothing to do.  Every wavefront reads the two words for itself; the decision is the
    // same in all of them because NOBODY writes either word before the barriers below (item 6f's rule: other workgroups write this tile's
    // flag of round r during round r + 1 only, this workgroup clears it at the very end; the plateau word is written by init alone)
    if (tld_load(cur + blockIdx.x) == 0 || tld_load(a.words + 2 * (size_t)a.g.B + p.b) != 0) return;
    const int tid = threadIdx.x, H = a.g.H, W = a.g.W;
    double* acc = a.acc + p.base;
    const uint8_t* succ = a.succ + p.base;
    // 2. load the tile: a halo cell outside the map is "no child"; A is read only where a value can be used
    if (tid < 8) flags[tid] = 0;
    for (int k = tid; k < kHaloH * kHaloW; k += kTileT) {
        const int ly = k / kHaloW, lx = k - ly * kHaloW;
        const int y = p.y0 - 1 + ly, x = p.x0 - 1 + lx;
        uint8_t s = kNoSucc;
        double v = 0.0;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const size_t i = (size_t)y * W + x;
            s = succ[i];
            if (s != kNoSucc) v = gtl_load(acc + i);
        }
        S[k] = s;
        A[k] = v;
    }
    __syncthreads();

    // 3. what this lane keeps of its cells: column tid % 64 of rows tid / 64, tid / 64 + 4, ... -- G, and the 8-bit set of its CHILDREN
    const int c = tid & (kTileW - 1), r0 = tid / kTileW;
    float g[K];
    uint32_t kids[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int r = r0 + k * kRowStep;
        const int q = (r + 1) * kHaloW + (c + 1);
        g[k] = 0.f;
        kids[k] = 0;
        if (S[q] != kNoSucc) {  // live (a cell outside the map or the ragged tile holds kNoSucc, and so does the halo beyond the map)
            kids[k] = fld_child_set([&](int dy, int dx) { return S[q + dy * kHaloW + dx]; }, true, true, true, true);
            if (kids[k]) g[k] = a.grad_dist[p.base + (size_t)(p.y0 + r) * W + (p.x0 + c)];
        }
    }

    // 4. the local fixed point on the interior, the halo fixed
    fld_sweep(flags, kTileH * kTileW, [&](bool backwards) {
        bool changed = false;
        double* q = A + (r0 + 1) * kHaloW + (c + 1);
        if (!backwards) {
#pragma unroll
            for (int k = 0; k < K; ++k) changed |= fld_subtree_sum(q + k * kRowStep * kHaloW, kHaloW, kids[k], g[k]);
        } else {
#pragma unroll
            for (int k = K - 1; k >= 0; --k) changed |= fld_subtree_sum(q + k * kRowStep * kHaloW, kHaloW, kids[k], g[k]);
        }
        return changed;
    });

    // 5. write back what changed (nobody else writes this tile's interior: HBM still holds what was loaded) and note which adjacent tile
    // reads it: the one that holds the cell's successor
    uint32_t edges = 0;  // bit 0 N, 1 S, 2 W, 3 E, 4 NW, 5 NE, 6 SW, 7 SE
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (kids[k]) {
            const int r = r0 + k * kRowStep;
            const int q = (r + 1) * kHaloW + (c + 1);
            const double v = A[q];
            double* d = acc + (size_t)(p.y0 + r) * W + (p.x0 + c);
            if (__double_as_longlong(v) != __double_as_longlong(gtl_load(d))) {
                gtl_store(d, v);
                const Move m = fld_move<kActionMoves>(S[q]);
                const int sy = r + m.dy, sx = c + m.dx;
                const bool n = sy < 0, so = sy >= p.rows, w = sx < 0, e = sx >= p.cols;
                edges |= (n && !w && !e ? 1u : 0u) | (so && !w && !e ? 2u : 0u) | (w && !n && !so ? 4u : 0u) | (e && !n && !so ? 8u : 0u) |
                         (n && w ? 16u : 0u) | (n && e ? 32u : 0u) | (so && w ? 64u : 0u) | (so && e ? 128u : 0u);
            }
        }
    }
    // 6. mark the adjacent tiles (a successor lies inside the map: the tile exists), and the map
    tld_end_round(a.g, p, edges, flags, cur, nxt, a.words, a.visits, round);
}

// last_round: the number of rounds launched; a map that marked a tile in that round still has an active one
__global__ __launch_bounds__(kTileT) void nastar_fields_grad_tiled_finish_kernel(const GradTiledArgs a, const int last_round)
{
    const TilePos p = tld_pos(a.g);
    const int tid = threadIdx.x, W = a.g.W;
    const bool plateau = tld_load(a.words + 2 * (size_t)a.g.B + p.b) != 0;
    const bool quiet = tld_map_quiet(a.words, p.b, last_round);
    if (p.t == 0 && tid == 0) a.status[p.b] = plateau ? NASTAR_ERR_PLATEAU : quiet ? NASTAR_OK : NASTAR_ERR_NO_CONVERGENCE;
    const bool write_sums = !plateau && quiet;  // a partial subtree sum is a bound of nothing: all zeros
    const int cc = tid & (kTileW - 1);
    if (cc >= p.cols) return;
    for (int rr = tid / kTileW; rr < p.rows; rr += kTileT / kTileW) {
        const size_t i = p.base + (size_t)(p.y0 + rr) * W + (p.x0 + cc);
        a.grad_cost[i] = (write_sums && a.succ[i] != kNoSucc) ? (float)gtl_load(a.acc + i) : 0.f;
    }
}

}  // namespace nastar
