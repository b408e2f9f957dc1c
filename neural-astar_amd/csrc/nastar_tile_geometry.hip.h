// nastar_tile_geometry.hip.h -- what the tiled kernels share (nastar_fields_tiled.hip.h, item 6f; nastar_fields_grad_tiled.hip.h, item 6h): the
// tile size, the grid of tiles and the position of a workgroup's tile, the accessors of the words that other workgroups write or have
// written (flags, per-map words): relaxed agent-scope atomics -- vector accesses, never the scalar path -- the end of a round
// (tld_end_round) and the verdict on a map (tld_map_quiet).  No kernel lives here, so that two translation units may include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nastar_field_rules.hip.h"

namespace nastar {

constexpr int kTiledMaxCells = 1179648;  // 1024 x 1152: the limit of the search entry points
constexpr int kTileH = 64, kTileW = 64;  // the interior of a tile: 16 cells per lane of a 256-lane workgroup, as in item 6e
constexpr int kTileT = 256;
constexpr int kHaloW = kTileW + 2, kHaloH = kTileH + 2;
static_assert(kTileW == 64 && kTileT % kTileW == 0, "a wavefront relaxes 64 consecutive cells of one tile row");
static_assert(kTileH * kTileW == kTileT * kFieldCellsPerLane, "a lane owns 16 cells of a tile, as in items 6e and 6g");

struct TileGrid {
    int B, H, W, ty, tx;    // ty x tx tiles per map
};

struct TiledArgs {
    const float* cost;      // [B,HW]
    const float* goal;
    const float* passable;
    float* dist;            // [B,HW]: the working field R, then the result
    float* policy;          // [B,8,HW] or nullptr
    int32_t* status;        // [B]
    int32_t* visits;        // [B] or nullptr
    int32_t* words;         // [4,B]: the last round in which the map marked a tile, the last round in which it relaxed one, has_goal, bad_cost
    int32_t* flags;         // [2,B*tiles]
    TileGrid g;
    uint32_t nmask;
};

__device__ __forceinline__ int tld_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void tld_store(int32_t* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// (map, tile row, tile column) of this workgroup and the map's first element
struct TilePos {
    int b, t, y0, x0, rows, cols;
    size_t base;
};
__device__ __forceinline__ TilePos tld_pos(const TileGrid& g)
{
    const int nt = g.ty * g.tx;
    TilePos p;
    p.b = (int)(blockIdx.x / (unsigned)nt);
    p.t = (int)(blockIdx.x - (unsigned)p.b * (unsigned)nt);
    const int tyi = p.t / g.tx, txi = p.t - tyi * g.tx;
    p.y0 = tyi * kTileH;
    p.x0 = txi * kTileW;
    p.rows = min(kTileH, g.H - p.y0);
    p.cols = min(kTileW, g.W - p.x0);
    p.base = (size_t)p.b * ((size_t)g.H * g.W);
    return p;
}

// the adjacent tile an edge bit stands for: bit 0 N, 1 S, 2 W, 3 E, 4 NW, 5 NE, 6 SW, 7 SE
constexpr Move kEdgeMoves[8] = {{-1, 0}, {1, 0}, {0, -1}, {0, 1}, {-1, -1}, {-1, 1}, {1, -1}, {1, 1}};

// THE END OF A ROUND of an active tile, every lane: `edges` = the adjacent tiles that have to look again, by this lane's cells.  ORs them
// into lds_flags[3]; marks, in the NEXT round's flags, those of them that exist (up to 8) and the map's word 0; then clears the tile's
// own flag of THIS round, which is this workgroup's to clear -- here, behind the barrier, when every wavefront has long read it -- and
// writes the map's word 1 and the visit.  cur / nxt: the flag arrays of this round and the next
__device__ __forceinline__ void tld_end_round(const TileGrid& g, const TilePos& p, uint32_t edges, int* lds_flags, int32_t* cur, int32_t* nxt,
                                              int32_t* words, int32_t* visits, int round)
{
    const int tid = threadIdx.x;
    if (edges) __hip_atomic_fetch_or(&lds_flags[3], (int)edges, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    if (tid < 8) {
        const Move m = fld_move<kEdgeMoves>(tid);
        const int tyi = p.t / g.tx, txi = p.t - tyi * g.tx;
        const int ny = tyi + m.dy, nx = txi + m.dx;
        if (((lds_flags[3] >> tid) & 1) && ny >= 0 && ny < g.ty && nx >= 0 && nx < g.tx) {
            tld_store(nxt + ((size_t)p.b * g.ty * g.tx + (size_t)(ny * g.tx + nx)), 1);
            tld_store(words + p.b, round);
        }
    }
    if (tid == 0) {
        tld_store(cur + blockIdx.x, 0);
        tld_store(words + (size_t)g.B + p.b, round);
        if (visits) atomicAdd(visits + p.b, 1);
    }
}

// THE VERDICT on a map after last_round rounds were launched: a map that marked a tile in that round still has an active one
__device__ __forceinline__ bool tld_map_quiet(const int32_t* words, int b, int last_round) { return last_round == 0 || tld_load(words + b) < last_round; }

}  // namespace nastar
