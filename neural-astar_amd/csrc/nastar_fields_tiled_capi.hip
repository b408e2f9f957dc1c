// nastar_fields_tiled_capi.hip -- the C ABI of include/nastar_fields_tiled.h: the cost-to-go field of maps of up to 1179648 cells by a tiled
// relaxation.  A translation unit of its own: nothing here touches the search, replay, encoder or one-workgroup field kernels.
#include <hip/hip_runtime.h>

#include "nastar_fields_tiled.hip.h"
#include "nastar_fields_host.hip.h"

using namespace nastar;

// rounds enqueued between two reads of the host (profiles/fields/probe_fields_tiled.jsonl holds the table over 1, 4, 8, 16: 1 is 2 to 5 %
// slower, the others are within 1.5 % of each other)
constexpr int kTiledLaunchesPerBatch = 8;

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
    return ((size_t)B * 16 + (size_t)B * (size_t)tile_count(H, W) * 8 + 15) / 16 * 16;
}

int nastar_cost_to_go_tiled_batched(const float* cost, const float* goal, const float* passable, int B, int H, int W, unsigned neighbor_mask,
                                    float* dist_out, float* policy_out, int32_t* status_out, int32_t* visits_out, void* workspace,
                                    size_t workspace_bytes, long long max_rounds, int launches_per_batch, int* rounds_out, void* stream)
{
    if (!field_mask_ok(neighbor_mask)) return NASTAR_ERR_UNSUPPORTED;
    if (!cost || !goal || !passable || !dist_out || !status_out || !workspace) return NASTAR_ERR_NULL;
    if (B < 1 || H < 1 || W < 1 || max_rounds < 0 || launches_per_batch < 0) return NASTAR_ERR_BAD_SHAPE;
    if (!tiled_shape_ok(B, H, W)) return NASTAR_ERR_UNSUPPORTED;
    if (workspace_bytes < nastar_cost_to_go_tiled_workspace_bytes(B, H, W) || (reinterpret_cast<uintptr_t>(workspace) & 3u) != 0) return NASTAR_ERR_WORKSPACE;

    const dim3 grid((unsigned)(B * tile_count(H, W)));
    int32_t* words = reinterpret_cast<int32_t*>(workspace);
    const TiledArgs a{cost, goal, passable, dist_out, policy_out, status_out, visits_out, words, words + (size_t)B * 4,
                      TileGrid{B, H, W, tiles_down(H), tiles_across(W)}, neighbor_mask};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int per_batch = launches_per_batch == 0 ? kTiledLaunchesPerBatch : launches_per_batch;

    int rc = clear_map_words(words, B, s);
    if (rc) return rc;
    rc = launch_grid(nastar_fields_tiled_init_kernel, grid, dim3(kTileT), 0, s, a);
    if (rc) return rc;
    const Rounds r = run_rounds(words, B, H, W, max_rounds, per_batch, s,
                                [&](int round) { return launch_grid(nastar_fields_tiled_round_kernel, grid, dim3(kTileT), 0, s, a, round); });
    if (r.rc) return r.rc;
    if (policy_out) {
        rc = launch_grid(nastar_fields_tiled_policy_kernel, grid, dim3(kTileT), 0, s, a);
        if (rc) return rc;
    }
    rc = launch_grid(nastar_fields_tiled_finish_kernel, grid, dim3(kTileT), 0, s, a, (int)r.launched);
    if (rc) return rc;
    if (rounds_out) *rounds_out = r.active_rounds;
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
