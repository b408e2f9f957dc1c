// nastar_tile_geometry.hip.h -- what the tiled kernels share (nastar_fields_tiled.hip.h, item 6f; nastar_fields_grad_tiled.hip.h, item 6h): the
// tile size, the arguments of the forward's kernels, the position of a workgroup's tile, and the accessors of the words that other
// workgroups write or have written (flags, per-map words): relaxed agent-scope atomics -- vector accesses, never the scalar path.  No kernel
// lives here, so that two translation units may include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nastar {

constexpr int kTiledMaxCells = 1179648;  // 1024 x 1152: the limit of the search entry points
constexpr int kTileH = 64, kTileW = 64;  // the interior of a tile: 16 cells per lane of a 256-lane workgroup, as in item 6e
constexpr int kTileT = 256;
constexpr int kHaloW = kTileW + 2, kHaloH = kTileH + 2;
static_assert(kTileW == 64 && kTileT % kTileW == 0, "a wavefront relaxes 64 consecutive cells of one tile row");

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
    int B, H, W, ty, tx;    // ty x tx tiles per map
    uint32_t nmask;
};

__device__ __forceinline__ int tld_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void tld_store(int32_t* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// (map, tile row, tile column) of this workgroup and the map's first element
struct TilePos {
    int b, t, y0, x0, rows, cols;
    size_t base;
};
__device__ __forceinline__ TilePos tld_pos(const TiledArgs& a)
{
    const int nt = a.ty * a.tx;
    TilePos p;
    p.b = (int)(blockIdx.x / (unsigned)nt);
    p.t = (int)(blockIdx.x - (unsigned)p.b * (unsigned)nt);
    const int tyi = p.t / a.tx, txi = p.t - tyi * a.tx;
    p.y0 = tyi * kTileH;
    p.x0 = txi * kTileW;
    p.rows = min(kTileH, a.H - p.y0);
    p.cols = min(kTileW, a.W - p.x0);
    p.base = (size_t)p.b * ((size_t)a.H * a.W);
    return p;
}

}  // namespace nastar
