// nastar_fields_host.hip.h -- what the host sides of the four field translation units share (nastar_fields*_capi.hip): the checks of the
// mask and of a tiled shape, the choice of the one-workgroup kernels' width, and the driver of the tiled kernels' rounds.
#pragma once
#include <algorithm>
#include <type_traits>
#include <vector>

#include "nastar_host.hip.h"
#include "nastar_tile_geometry.hip.h"

namespace nastar {

inline bool field_mask_ok(unsigned neighbor_mask) { return (neighbor_mask & ~0x1FFu) == 0u && (neighbor_mask & 0x10u) == 0u; }

inline int tiles_down(int H) { return (H + kTileH - 1) / kTileH; }
inline int tiles_across(int W) { return (W + kTileW - 1) / kTileW; }
inline long long tile_count(int H, int W) { return (long long)tiles_down(H) * tiles_across(W); }

inline bool tiled_shape_ok(int B, int H, int W)
{
    return B >= 1 && H >= 1 && W >= 1 && (long long)H * W <= kTiledMaxCells && (long long)B * tile_count(H, W) <= (1ll << 24);   // (x 256 lanes: the 2^32 threads a grid may have)
}

// f(integral_constant<int, T>) for the width T of the workgroup that owns a map of HW cells: one wavefront up to 1024 cells (the barrier
// of a sweep costs nothing), 4 up to 4096, 16 above -- at most kFieldCellsPerLane cells per lane at every limit
template <typename F>
inline int with_field_block(int HW, F&& f)
{
    if (HW <= 64 * kFieldCellsPerLane) return f(std::integral_constant<int, 64>{});
    if (HW <= 256 * kFieldCellsPerLane) return f(std::integral_constant<int, 256>{});
    return f(std::integral_constant<int, 1024>{});
}

// the four per-map words of a tiled call (a block of B x 16 bytes) start at zero
inline int clear_map_words(int32_t* words, int B, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(words, 0, (size_t)B * 16, s);
    return e == hipSuccess ? NASTAR_OK : hip_fail(e, "hipMemsetAsync(per-map words)");
}

// The rounds of a tiled call, behind its init launch: enqueue(r) launches round r = 1, 2, ... (-> a status); after every batch of
// per_batch rounds the host reads words[0..B), the last round in which the map marked a tile, and words[B..2B), the last round in which
// it worked on one.  Ends when nobody marked a tile in a batch's last round, or at the limit: max_rounds (0 = none) or the bound H*W + 1,
// since every round with an active tile makes one more cell final.
struct Rounds {
    int rc;
    long long launched;
    int active_rounds;
};
template <typename Enqueue>
inline Rounds run_rounds(const int32_t* words, int B, int H, int W, long long max_rounds, int per_batch, hipStream_t s, Enqueue&& enqueue)
{
    const long long bound = (long long)H * W + 1;
    const long long limit = max_rounds == 0 ? bound : std::min(max_rounds, bound);
    std::vector<int32_t> host((size_t)B * 2);
    Rounds r{NASTAR_OK, 0, 0};
    bool quiet = false;
    while (!quiet && r.launched < limit) {
        const long long n = std::min((long long)per_batch, limit - r.launched);
        for (long long k = 0; k < n; ++k) {
            r.rc = enqueue((int)(r.launched + 1));
            if (r.rc) return r;
            ++r.launched;
        }
        hipError_t e = hipMemcpyAsync(host.data(), words, host.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) return Rounds{hip_fail(e, "hipMemcpyAsync(per-map words)"), r.launched, r.active_rounds};
        e = hipStreamSynchronize(s);
        if (e != hipSuccess) return Rounds{hip_fail(e, "hipStreamSynchronize"), r.launched, r.active_rounds};
        quiet = *std::max_element(host.begin(), host.begin() + B) < r.launched;   // nobody marked a tile in the batch's last round
        r.active_rounds = *std::max_element(host.begin() + B, host.end());
    }
    return r;
}

}  // namespace nastar
