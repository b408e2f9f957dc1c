// nastar_fields_tiled_capi.hip -- the C ABI of include/nastar_fields_tiled.h: the cost-to-go field of maps of up to 1179648 cells by a tiled
// relaxation.  A translation unit of its own: nothing here touches the search, replay, encoder or one-workgroup field kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "nastar_fields_tiled.hip.h"
#include "nastar_host.hip.h"

using namespace nastar;

// rounds enqueued between two reads of the host (profiles/fields/probe_fields_tiled.jsonl holds the table over 1, 4, 8, 16: 1 is 2 to 5 %
// slower, the others are within 1.5 % of each other)
constexpr int kTiledLaunchesPerBatch = 8;

static inline long long tiled_tiles(int H, int W) { return (long long)((H + kTileH - 1) / kTileH) * ((W + kTileW - 1) / kTileW); }

static inline bool tiled_shape_ok(int B, int H, int W)
{
    return B >= 1 && H >= 1 && W >= 1 && (long long)H * W <= kTiledMaxCells && (long long)B * tiled_tiles(H, W) <= (1ll << 24);   // (x 256 lanes: the 2^32 threads a grid may have)
}

extern "C" {

int nastar_fields_tiled_abi(void) { return NASTAR_FIELDS_TILED_ABI; }

int nastar_fields_tiled_max_cells(void) { return kTiledMaxCells; }

int nastar_fields_tile(int* th, int* tw)
{
    if (!th || !tw) return NASTAR_ERR_NULL;
    *th = kTileH;
    *tw = kTileW;
    return NASTAR_OK;
}

size_t nastar_cost_to_go_tiled_workspace_bytes(int B, int H, int W)
{
    if (!tiled_shape_ok(B, H, W)) return 0;
    // the four per-map words first (a block of B x 16 bytes, zeroed by one memset), then the two flag arrays
    return ((size_t)B * 16 + (size_t)B * (size_t)tiled_tiles(H, W) * 8 + 15) / 16 * 16;
}

int nastar_cost_to_go_tiled_batched(const float* cost, const float* goal, const float* passable, int B, int H, int W, unsigned neighbor_mask,
                                    float* dist_out, float* policy_out, int32_t* status_out, int32_t* visits_out, void* workspace,
                                    size_t workspace_bytes, long long max_rounds, int launches_per_batch, int* rounds_out, void* stream)
{
    if ((neighbor_mask & ~0x1FFu) != 0u || (neighbor_mask & 0x10u) != 0u) return NASTAR_ERR_UNSUPPORTED;
    if (!cost || !goal || !passable || !dist_out || !status_out || !workspace) return NASTAR_ERR_NULL;
    if (B < 1 || H < 1 || W < 1 || max_rounds < 0 || launches_per_batch < 0) return NASTAR_ERR_BAD_SHAPE;
    if (!tiled_shape_ok(B, H, W)) return NASTAR_ERR_UNSUPPORTED;
    if (workspace_bytes < nastar_cost_to_go_tiled_workspace_bytes(B, H, W) || (reinterpret_cast<uintptr_t>(workspace) & 3u) != 0) return NASTAR_ERR_WORKSPACE;

    const int ty = (H + kTileH - 1) / kTileH, tx = (W + kTileW - 1) / kTileW;
    const dim3 grid((unsigned)((long long)B * ty * tx));
    int32_t* words = reinterpret_cast<int32_t*>(workspace);
    const TiledArgs a{cost, goal, passable, dist_out, policy_out, status_out, visits_out, words, words + (size_t)B * 4, B, H, W, ty, tx, neighbor_mask};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long bound = (long long)H * W + 1;  // every round with an active tile makes one more cell final
    const long long limit = max_rounds == 0 ? bound : std::min(max_rounds, bound);
    const int per_batch = launches_per_batch == 0 ? kTiledLaunchesPerBatch : launches_per_batch;

    hipError_t e = hipMemsetAsync(words, 0, (size_t)B * 16, s);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(per-map words)");
    int rc = launch_grid(nastar_fields_tiled_init_kernel, grid, dim3(kTileT), 0, s, a);
    if (rc) return rc;

    // words[0..B): the last round in which the map marked a tile; words[B..2B): the last round in which it relaxed one
    std::vector<int32_t> host((size_t)B * 2);
    long long launched = 0;
    int active_rounds = 0;
    bool quiet = false;
    while (!quiet && launched < limit) {
        const long long n = std::min((long long)per_batch, limit - launched);
        for (long long k = 0; k < n; ++k) {
            rc = launch_grid(nastar_fields_tiled_round_kernel, grid, dim3(kTileT), 0, s, a, (int)(launched + 1));
            if (rc) return rc;
            ++launched;
        }
        e = hipMemcpyAsync(host.data(), words, host.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(per-map words)");
        e = hipStreamSynchronize(s);
        if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
        quiet = *std::max_element(host.begin(), host.begin() + B) < launched;   // nobody marked a tile in the batch's last round
        active_rounds = *std::max_element(host.begin() + B, host.end());
    }
    if (policy_out) {
        rc = launch_grid(nastar_fields_tiled_policy_kernel, grid, dim3(kTileT), 0, s, a);
        if (rc) return rc;
    }
    rc = launch_grid(nastar_fields_tiled_finish_kernel, grid, dim3(kTileT), 0, s, a, (int)launched);
    if (rc) return rc;
    if (rounds_out) *rounds_out = active_rounds;
    return NASTAR_OK;
}

int nastar_cost_to_go_tiled(const float* cost, const float* goal, const float* passable, int B, int H, int W, unsigned neighbor_mask,
                            float* dist_out, float* policy_out, int32_t* status_out, int32_t* visits_out, void* workspace, size_t workspace_bytes,
                            long long max_rounds, int* rounds_out, void* stream)
{
    return nastar_cost_to_go_tiled_batched(cost, goal, passable, B, H, W, neighbor_mask, dist_out, policy_out, status_out, visits_out, workspace,
                                           workspace_bytes, max_rounds, 0, rounds_out, stream);
}

}  // extern "C"
