// nastar_fields_tiled.hip.h -- the cost-to-go field of maps too large for one workgroup: a tiled relaxation of the definition of
// include/nastar_fields.h (include/nastar_fields_tiled.h).
//
// The working field R of item 6e (0 on passable goals, +inf elsewhere at the start, only ever lowered) lives in dist_out, in HBM.  The map
// is cut into tiles of kTileH x kTileW cells.  Four kernels, one workgroup per (map, tile) each:
//   init    writes R, finds NaN / negative costs and goals per map, and marks the tiles that start active: every tile whose interior PLUS
//           one-cell halo holds a passable goal (a goal in a border cell whose in-tile neighbours are obstacles lowers nothing in its own
//           tile, only in the next one);
//   round   a tile that is not active this round exits.  An active one loads its interior and a one-cell
//           halo of R (+inf outside the map) and C (cost, obstacles folded in as +inf) into LDS, relaxes the interior to the LOCAL fixed
//           point with fld_sweep (bounded by the tile's cell count), stores the cells it lowered and ends the round with tld_end_round
//           on every existing adjacent tile whose halo holds one of them (up to 8);
//   policy  the eight planes, fld_best_action on the converged R (a goal on an obstacle is still +inf there, as in 6e);
//   finish  the goal cells (0, passable or not), all +inf for a map with a bad cost, and the status.
// Inside a launch nothing is handed from one workgroup to another: every value a workgroup reads from another tile, old or new, is an upper
// bound of the fixed point (a 32-bit word is never torn), and a tile that read a stale halo has been marked by the writer and reads it
// again after a kernel boundary.  Two flag arrays alternate: a tile's flag of round r is read and, at the end, cleared by its own workgroup
// in round r and written by others during round r + 1 only.  The words other workgroups write or have written (flags, per-map words) are read and written
// through relaxed agent-scope atomics: vector accesses, never the scalar path.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nastar_fields_tiled.h"
#include "nastar_fields.hip.h"
#include "nastar_tile_geometry.hip.h"

namespace nastar {

__global__ __launch_bounds__(kTileT) void nastar_fields_tiled_init_kernel(const TiledArgs a)
{
    const TilePos p = tld_pos(a.g);
    const int tid = threadIdx.x, H = a.g.H, W = a.g.W;
    const float* cost = a.cost + p.base;
    const float* goal = a.goal + p.base;
    const float* pass = a.passable + p.base;
    float* dist = a.dist + p.base;
    bool near_goal = false, has_goal = false, bad = false;
    for (int k = tid; k < kHaloH * kHaloW; k += kTileT) {
        const int ly = k / kHaloW, lx = k - ly * kHaloW;
        const int y = p.y0 - 1 + ly, x = p.x0 - 1 + lx;
        if (y < 0 || y >= H || x < 0 || x >= W) continue;
        const int i = y * W + x;
        const float g = goal[i];
        const bool ok = pass[i] != 0.f;
        near_goal |= ok && g != 0.f;
        if (ly >= 1 && ly <= kTileH && lx >= 1 && lx <= kTileW) {   // the interior: this workgroup's own cells
            const float c = cost[i];
            bad |= ok && !(c >= 0.f);             // NaN or negative on a passable cell (-0.0 >= 0)
            has_goal |= g != 0.f;
            dist[i] = (ok && g != 0.f) ? 0.f : INFINITY;
        }
    }
    const int any_near = __syncthreads_or(near_goal), any_goal = __syncthreads_or(has_goal), any_bad = __syncthreads_or(bad);
    if (tid == 0) {
        const size_t nflags = (size_t)a.g.B * a.g.ty * a.g.tx;
        tld_store(a.flags + blockIdx.x, any_near ? 1 : 0);
        tld_store(a.flags + nflags + blockIdx.x, 0);
        if (any_goal) tld_store(a.words + 2 * (size_t)a.g.B + p.b, 1);
        if (any_bad) tld_store(a.words + 3 * (size_t)a.g.B + p.b, 1);
        if (p.t == 0 && a.visits) a.visits[p.b] = 0;
    }
}

// round: 1, 2, ... ; the flags of round r are array (r - 1) & 1
__global__ __launch_bounds__(kTileT) void nastar_fields_tiled_round_kernel(const TiledArgs a, const int round)
{
    __shared__ float R[kHaloH * kHaloW];          // interior + halo; the halo is never written
    __shared__ float C[kTileH * kTileW];
    __shared__ int flags[8];                      // [0..2] sweep flags, [3] the borders that hold a lowered cell
    const size_t nflags = (size_t)a.g.B * a.g.ty * a.g.tx;
    int32_t* cur = a.flags + (size_t)((round - 1) & 1) * nflags;
    int32_t* nxt = a.flags + (size_t)(round & 1) * nflags;
    const TilePos p = tld_pos(a.g);
    // 1. not active this round, or a map with a bad cost: nothing to do.  Every wavefront reads the two words for itself, so the decision is
    // the same in all of them only because NOBODY writes either word before the barriers below: other workgroups write this tile's flag of
    // round r during round r + 1 only, and this workgroup clears it at the very end, behind barriers every wavefront has passed
    if (tld_load(cur + blockIdx.x) == 0 || tld_load(a.words + 3 * (size_t)a.g.B + p.b) != 0) return;
    const int tid = threadIdx.x, H = a.g.H, W = a.g.W;
    const float INF = INFINITY;
    float* dist = a.dist + p.base;
    const float* cost = a.cost + p.base;
    const float* pass = a.passable + p.base;
    // 2. load the tile
    if (tid < 8) flags[tid] = 0;
    for (int k = tid; k < kHaloH * kHaloW; k += kTileT) {
        const int ly = k / kHaloW, lx = k - ly * kHaloW;
        const int y = p.y0 - 1 + ly, x = p.x0 - 1 + lx;
        R[k] = (y >= 0 && y < H && x >= 0 && x < W) ? dist[y * W + x] : INF;
    }
    for (int k = tid; k < kTileH * kTileW; k += kTileT) {
        const int ly = k / kTileW, lx = k - ly * kTileW;
        const int y = p.y0 + ly, x = p.x0 + lx;
        float c = INF;
        if (y < H && x < W) {
            const int i = y * W + x;
            if (pass[i] != 0.f) c = cost[i];
        }
        C[k] = c;
    }
    __syncthreads();

    // 3. the local fixed point on the interior.  Lane l owns column l % 64 of rows l / 64, l / 64 + 4, ...
    const uint32_t nm = a.nmask;
    const int c = tid & (kTileW - 1), r0 = tid / kTileW;
    constexpr int kRowStep = kTileT / kTileW;
    const int nk = (c < p.cols && r0 < p.rows) ? (p.rows - r0 + kRowStep - 1) / kRowStep : 0;
    auto relax = [&](int r) -> bool {
        float* q = R + (r + 1) * kHaloW + (c + 1);
        float m = INF;
        fld_each<8>([&](auto j) __attribute__((always_inline)) {
            constexpr Move o = kChildOffsets[decltype(j)::value];
            if (nm & fld_bit(o.dy, o.dx)) m = fminf(m, fld_load(q + o.dy * kHaloW + o.dx));
        });
        const float cand = C[r * kTileW + c] + m;
        if (cand < fld_load(q)) {
            fld_store(q, cand);
            return true;
        }
        return false;
    };
    fld_sweep(flags, kTileH * kTileW, [&](bool backwards) {
        bool changed = false;
        if (!backwards) {
            for (int k = 0; k < nk; ++k) changed |= relax(r0 + k * kRowStep);
        } else {
            for (int k = nk - 1; k >= 0; --k) changed |= relax(r0 + k * kRowStep);
        }
        return changed;
    });

    // 4. write back what was lowered (nobody else writes this tile's interior: dist still holds what was loaded) and note the borders
    uint32_t edges = 0;   // bit 0 N, 1 S, 2 W, 3 E, 4 NW, 5 NE, 6 SW, 7 SE
    for (int k = 0; k < nk; ++k) {
        const int r = r0 + k * kRowStep;
        const float v = R[(r + 1) * kHaloW + (c + 1)];
        float* d = dist + (size_t)(p.y0 + r) * W + (p.x0 + c);
        if (v < *d) {
            *d = v;
            const bool n = r == 0, s = r == p.rows - 1, w = c == 0, e = c == p.cols - 1;
            edges |= (n ? 1u : 0u) | (s ? 2u : 0u) | (w ? 4u : 0u) | (e ? 8u : 0u) | (n && w ? 16u : 0u) | (n && e ? 32u : 0u) |
                     (s && w ? 64u : 0u) | (s && e ? 128u : 0u);
        }
    }
    // 5, 6. mark the adjacent tiles that exist, and the map
    tld_end_round(a.g, p, edges, flags, cur, nxt, a.words, a.visits, round);
}

// the policy planes from the converged R; a map with a bad cost gets zeros
__global__ __launch_bounds__(kTileT) void nastar_fields_tiled_policy_kernel(const TiledArgs a)
{
    const TilePos p = tld_pos(a.g);
    const int tid = threadIdx.x, H = a.g.H, W = a.g.W;
    const size_t HW = (size_t)H * W;
    const float* R = a.dist + p.base;
    float* pol = a.policy + p.base * 8;
    const bool map_bad = tld_load(a.words + 3 * (size_t)a.g.B + p.b) != 0;
    const uint32_t nm = a.nmask;
    const float INF = INFINITY;
    const int cc = tid & (kTileW - 1);
    if (cc >= p.cols) return;
    const int x = p.x0 + cc;
    for (int rr = tid / kTileW; rr < p.rows; rr += kTileT / kTileW) {
        const int y = p.y0 + rr;
        const ptrdiff_t i = (ptrdiff_t)y * W + x;
        const float d = map_bad ? INF : R[i];
        int best = -1;
        if (d > 0.f && d < INF)
            best = fld_best_action([&](int dy, int dx) { return R[i + (ptrdiff_t)dy * W + dx]; }, nm, y > 0, y < H - 1, x > 0, x < W - 1, d);
#pragma unroll
        for (int k = 0; k < 8; ++k) pol[(size_t)k * HW + (size_t)i] = (k == best) ? 1.f : 0.f;
    }
}

// after the policy launch (which reads R, where a goal on an obstacle is +inf): the goal cells, the maps with a bad cost, the status.
// last_round: the number of rounds launched; a map that marked a tile in that round still has an active one
__global__ __launch_bounds__(kTileT) void nastar_fields_tiled_finish_kernel(const TiledArgs a, const int last_round)
{
    const TilePos p = tld_pos(a.g);
    const int tid = threadIdx.x, W = a.g.W;
    const float* goal = a.goal + p.base;
    float* dist = a.dist + p.base;
    const bool map_bad = tld_load(a.words + 3 * (size_t)a.g.B + p.b) != 0;
    if (p.t == 0 && tid == 0) {
        const bool map_goal = tld_load(a.words + 2 * (size_t)a.g.B + p.b) != 0;
        const bool quiet = tld_map_quiet(a.words, p.b, last_round);
        a.status[p.b] = map_bad ? NASTAR_ERR_BAD_COST : !map_goal ? NASTAR_ERR_UNSOLVABLE : quiet ? NASTAR_OK : NASTAR_ERR_NO_CONVERGENCE;
    }
    const int cc = tid & (kTileW - 1);
    if (cc >= p.cols) return;
    for (int rr = tid / kTileW; rr < p.rows; rr += kTileT / kTileW) {
        const size_t i = (size_t)(p.y0 + rr) * W + (p.x0 + cc);
        if (map_bad) dist[i] = INFINITY;
        else if (goal[i] != 0.f) dist[i] = 0.f;
    }
}

}  // namespace nastar
