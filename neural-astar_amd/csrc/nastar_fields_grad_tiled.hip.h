// nastar_fields_grad_tiled.hip.h -- the gradient of the cost-to-go field with respect to the cost maps for maps too large for one workgroup:
// the subtree sum of include/nastar_fields_grad.h, tiled (include/nastar_fields_grad_tiled.h).
//
// Definition, rounding rule and summation order are those of nastar_fields_grad.hip.h (item 6g); the geometry is that of
// nastar_fields_tiled.hip.h (item 6f): tiles of kTileH x kTileW cells, one 256-lane workgroup per (map, tile), two alternating flag arrays,
// per-map words.  The workspace holds, per cell, the fp64 accumulator A (8 B) and one successor byte.  Three kernels:
//   init    per cell: live or not, and the successor (the policy of nastar_fields_tiled_policy_kernel on the readable field, one-cell halo
//           read from HBM); writes the successor byte, A = G on live cells and 0 elsewhere, raises the map's plateau word for a live cell
//           without a successor, marks the tile active when it holds a live cell;
//   round   a tile that is not active, or whose map has the plateau word, exits.  An active one loads A and the successor bytes, interior
//           plus a one-cell halo ("no child" outside the map), into LDS; a lane keeps G and the 8-bit child set of its 16 cells in
//           registers; the sweep loop of items 6e / 6g recomputes IN PLACE every cell that has a child, A(v) = G(v) + A(c_0) + ..., children
//           in row-major order, to the LOCAL fixed point (halo fixed; bounded by the tile's cell count); then it stores the interior cells
//           whose bits differ from what HBM holds, marks, in the NEXT round's flags, the adjacent tile that holds the successor of such a
//           cell (the only tile that reads it), and clears its own flag as its last act;
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
static_assert(kTileH * kTileW == kTileT * kGradCellsPerLane, "a lane owns 16 cells of a tile, as in item 6g");

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
    int B, H, W, ty, tx;
    uint32_t nmask;
};

__device__ __forceinline__ double gtl_load(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void gtl_store(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ TilePos gtl_pos(const GradTiledArgs& a)
{
    TiledArgs t{};
    t.B = a.B, t.H = a.H, t.W = a.W, t.ty = a.ty, t.tx = a.tx;
    return tld_pos(t);
}

__global__ __launch_bounds__(kTileT) void nastar_fields_grad_tiled_init_kernel(const GradTiledArgs a)
{
    const TilePos p = gtl_pos(a);
    const int tid = threadIdx.x, H = a.H, W = a.W;
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
                const bool up = y > 0, dn = y < H - 1, lf = x > 0, rt = x < W - 1;
                float m = INF;
                // synthetic.ACTION_MOVES order on the READABLE field; a strict < keeps the first action among equals
#define NASTAR_GTL_ACT(k, dy, dx, ok)                                            \
    if ((nm & fld_bit(dy, dx)) && (ok)) {                                         \
        const ptrdiff_t j = i + (ptrdiff_t)(dy) * W + (dx);                       \
        const float v = pass[j] != 0.f ? dist[j] : INF;                           \
        if (v < m) {                                                              \
            m = v;                                                                \
            best = k;                                                             \
        }                                                                         \
    }
                NASTAR_GTL_ACT(0, -1, 0, up)
                NASTAR_GTL_ACT(1, 0, 1, rt)
                NASTAR_GTL_ACT(2, 0, -1, lf)
                NASTAR_GTL_ACT(3, 1, 0, dn)
                NASTAR_GTL_ACT(4, -1, 1, up && rt)
                NASTAR_GTL_ACT(5, -1, -1, up && lf)
                NASTAR_GTL_ACT(6, 1, 1, dn && rt)
                NASTAR_GTL_ACT(7, 1, -1, dn && lf)
#undef NASTAR_GTL_ACT
                if (!(m < d)) best = -1;
                stuck |= best < 0;
                any_live = true;
            }
            a.succ[p.base + (size_t)i] = best < 0 ? kNoSucc : (uint8_t)best;
            if (a.grad_dist) gtl_store(a.acc + p.base + (size_t)i, live ? (double)a.grad_dist[p.base + (size_t)i] : 0.0);
        }
    }
    const int tile_live = __syncthreads_or(any_live), tile_stuck = __syncthreads_or(stuck);
    if (tid == 0) {
        const size_t nflags = (size_t)a.B * a.ty * a.tx;
        tld_store(a.flags + blockIdx.x, tile_live ? 1 : 0);
        tld_store(a.flags + nflags + blockIdx.x, 0);
        if (tile_stuck) tld_store(a.words + 2 * (size_t)a.B + p.b, 1);
        if (p.t == 0 && a.visits) a.visits[p.b] = 0;
    }
}

// the plateau verdict alone: behind an init launch
__global__ __launch_bounds__(kTileT) void nastar_fields_grad_tiled_status_kernel(const GradTiledArgs a)
{
    const size_t b = (size_t)blockIdx.x * kTileT + threadIdx.x;
    if (b < (size_t)a.B) a.status[b] = tld_load(a.words + 2 * (size_t)a.B + b) != 0 ? NASTAR_ERR_PLATEAU : NASTAR_OK;
}

// round: 1, 2, ... ; the flags of round r are array (r - 1) & 1
__global__ __launch_bounds__(kTileT) void nastar_fields_grad_tiled_round_kernel(const GradTiledArgs a, const int round)
{
    __shared__ double A[kHaloH * kHaloW];           // interior + halo; the halo is never written
    __shared__ uint8_t S[kHaloH * kHaloW + 4];      // the successor bytes of the same cells
    __shared__ int flags[8];                        // [0..2] sweep flags, [3] the adjacent tiles that read a cell this one changed
    constexpr int K = kGradCellsPerLane;
    constexpr int kRowStep = kTileT / kTileW;
    const size_t nflags = (size_t)a.B * a.ty * a.tx;
    int32_t* cur = a.flags + (size_t)((round - 1) & 1) * nflags;
    int32_t* nxt = a.flags + (size_t)(round & 1) * nflags;
    const TilePos p = gtl_pos(a);
    // 1. not active this round, or a map with a plateau: nothing to do.  Every wavefront reads the two words for itself; the decision is the
    // same in all of them because NOBODY writes either word before the barriers below (item 6f's rule: other workgroups write this tile's
    // flag of round r during round r + 1 only, this workgroup clears it at the very end; the plateau word is written by init alone)
    if (tld_load(cur + blockIdx.x) == 0 || tld_load(a.words + 2 * (size_t)a.B + p.b) != 0) return;
    const int tid = threadIdx.x, H = a.H, W = a.W;
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
    // (bit j: the neighbour at the j-th offset of the header's row-major order steps onto this cell; its action is the opposite move)
    const int c = tid & (kTileW - 1), r0 = tid / kTileW;
    float g[K];
    uint32_t kids[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int r = r0 + k * kRowStep;
        const int q = (r + 1) * kHaloW + (c + 1);
        g[k] = 0.f;
        uint32_t m = 0;
        if (S[q] != kNoSucc) {  // live (a cell outside the map or the ragged tile holds kNoSucc)
#define NASTAR_GTL_KID(j, dy, dx, act) \
    if (S[q + (dy) * kHaloW + (dx)] == (act)) m |= 1u << (j);
            NASTAR_GTL_KID(0, -1, -1, 6)
            NASTAR_GTL_KID(1, -1, 0, 3)
            NASTAR_GTL_KID(2, -1, 1, 7)
            NASTAR_GTL_KID(3, 0, -1, 1)
            NASTAR_GTL_KID(4, 0, 1, 2)
            NASTAR_GTL_KID(5, 1, -1, 4)
            NASTAR_GTL_KID(6, 1, 0, 0)
            NASTAR_GTL_KID(7, 1, 1, 5)
#undef NASTAR_GTL_KID
            if (m) g[k] = a.grad_dist[p.base + (size_t)(p.y0 + r) * W + (p.x0 + c)];
        }
        kids[k] = m;
    }

    // 4. the local fixed point: the sweep loop of item 6g on the interior, the halo fixed
    for (int s = 0; s < kTileH * kTileW; ++s) {  // the bound: no input moves it
        bool changed = false;
        auto visit = [&](int k) {
            const uint32_t m = kids[k];
            if (m) {
                double* q = A + (r0 + k * kRowStep + 1) * kHaloW + (c + 1);
                double v = (double)g[k];
#define NASTAR_GTL_ADD(j, dy, dx) \
    if (m & (1u << (j))) v += fgr_load(q + (dy) * kHaloW + (dx));
                NASTAR_GTL_ADD(0, -1, -1)
                NASTAR_GTL_ADD(1, -1, 0)
                NASTAR_GTL_ADD(2, -1, 1)
                NASTAR_GTL_ADD(3, 0, -1)
                NASTAR_GTL_ADD(4, 0, 1)
                NASTAR_GTL_ADD(5, 1, -1)
                NASTAR_GTL_ADD(6, 1, 0)
                NASTAR_GTL_ADD(7, 1, 1)
#undef NASTAR_GTL_ADD
                if (__double_as_longlong(v) != __double_as_longlong(fgr_load(q))) {
                    fgr_store(q, v);
                    changed = true;
                }
            }
        };
        if ((s & 1) == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) visit(k);
        } else {
#pragma unroll
            for (int k = K - 1; k >= 0; --k) visit(k);
        }
        const int slot = s % 3;
        if (__ballot(changed) && (tid & 63) == 0) __hip_atomic_store(&flags[slot], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (tid == 0) __hip_atomic_store(&flags[slot == 2 ? 0 : slot + 1], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __syncthreads();
        if (__hip_atomic_load(&flags[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0) break;
    }

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
                const int act = S[q];  // ACTION_MOVES: (-1,0) (0,1) (0,-1) (1,0) (-1,1) (-1,-1) (1,1) (1,-1)
                const int dy = (act == 0 || act == 4 || act == 5) ? -1 : (act == 3 || act == 6 || act == 7) ? 1 : 0;
                const int dx = (act == 2 || act == 5 || act == 7) ? -1 : (act == 1 || act == 4 || act == 6) ? 1 : 0;
                const int sy = r + dy, sx = c + dx;
                const bool n = sy < 0, so = sy >= p.rows, w = sx < 0, e = sx >= p.cols;
                edges |= (n && !w && !e ? 1u : 0u) | (so && !w && !e ? 2u : 0u) | (w && !n && !so ? 4u : 0u) | (e && !n && !so ? 8u : 0u) |
                         (n && w ? 16u : 0u) | (n && e ? 32u : 0u) | (so && w ? 64u : 0u) | (so && e ? 128u : 0u);
            }
        }
    }
    if (edges) __hip_atomic_fetch_or(&flags[3], (int)edges, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    // 6. mark the adjacent tiles (a successor lies inside the map: the tile exists; the test stays, it costs nothing), and the map
    if (tid < 8) {
        const int dy = (tid == 0 || tid == 4 || tid == 5) ? -1 : (tid == 1 || tid == 6 || tid == 7) ? 1 : 0;
        const int dx = (tid == 2 || tid == 4 || tid == 6) ? -1 : (tid == 3 || tid == 5 || tid == 7) ? 1 : 0;
        const int tyi = p.t / a.tx, txi = p.t - tyi * a.tx;
        const int ny = tyi + dy, nx = txi + dx;
        if (((flags[3] >> tid) & 1) && ny >= 0 && ny < a.ty && nx >= 0 && nx < a.tx) {
            tld_store(nxt + ((size_t)p.b * a.ty * a.tx + (size_t)(ny * a.tx + nx)), 1);
            tld_store(a.words + p.b, round);
        }
    }
    if (tid == 0) {
        // the flag of this round is this workgroup's to clear -- here, after the barriers, when every wavefront has long read it
        tld_store(cur + blockIdx.x, 0);
        tld_store(a.words + (size_t)a.B + p.b, round);
        if (a.visits) atomicAdd(a.visits + p.b, 1);
    }
}

// last_round: the number of rounds launched; a map that marked a tile in that round still has an active one
__global__ __launch_bounds__(kTileT) void nastar_fields_grad_tiled_finish_kernel(const GradTiledArgs a, const int last_round)
{
    const TilePos p = gtl_pos(a);
    const int tid = threadIdx.x, W = a.W;
    const bool plateau = tld_load(a.words + 2 * (size_t)a.B + p.b) != 0;
    const bool quiet = last_round == 0 || tld_load(a.words + p.b) < last_round;
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
