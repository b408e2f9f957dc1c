// nastar_fields_grad_tiled_capi.hip -- the C ABI of include/nastar_fields_grad_tiled.h: the gradient of the cost-to-go field with respect to
// the cost maps for maps of up to 1179648 cells, by a tiled subtree sum.  A translation unit of its own: nothing here touches the search,
// replay, encoder, forward field or one-workgroup gradient kernels.
#include <hip/hip_runtime.h>

#include "nastar_fields_grad_tiled.hip.h"
#include "nastar_fields_host.hip.h"

using namespace nastar;

// rounds enqueued between two reads of the host: the forward's choice (nastar_fields_tiled_capi.hip)
constexpr int kGradTiledLaunchesPerBatch = 8;

// the refusals both entry points share, in the header's order, and the arguments of the kernels
static int gtl_args(const float* dist, const float* goal, const float* passable, const float* grad_dist, bool want_grad, int B, int H, int W,
                    unsigned neighbor_mask, float* grad_cost_out, int32_t* status_out, int32_t* visits_out, void* workspace, size_t workspace_bytes,
                    long long max_rounds, GradTiledArgs* out)
{
    if (!field_mask_ok(neighbor_mask)) return NASTAR_ERR_UNSUPPORTED;
    if (!dist || !goal || !passable || !status_out || !workspace || (want_grad && (!grad_dist || !grad_cost_out))) return NASTAR_ERR_NULL;
    if (B < 1 || H < 1 || W < 1 || max_rounds < 0) return NASTAR_ERR_BAD_SHAPE;
    if (!tiled_shape_ok(B, H, W)) return NASTAR_ERR_UNSUPPORTED;
    if (workspace_bytes < nastar_fields_backward_tiled_workspace_bytes(B, H, W) || (reinterpret_cast<uintptr_t>(workspace) & 7u) != 0) return NASTAR_ERR_WORKSPACE;
    // A first (8-byte words), then the four per-map words (a block of B x 16 bytes, zeroed by one memset), the two flag arrays, the successor bytes
    const size_t cells = (size_t)B * H * W, tiles = (size_t)B * (size_t)tile_count(H, W);
    char* w = reinterpret_cast<char*>(workspace);
    double* acc = reinterpret_cast<double*>(w);
    int32_t* words = reinterpret_cast<int32_t*>(w + cells * 8);
    int32_t* flags = words + (size_t)B * 4;
    uint8_t* succ = reinterpret_cast<uint8_t*>(flags + tiles * 2);
    *out = GradTiledArgs{dist, goal, passable, grad_dist, grad_cost_out, status_out, visits_out, acc, succ, words, flags,
                         TileGrid{B, H, W, tiles_down(H), tiles_across(W)}, neighbor_mask};
    return NASTAR_OK;
}

extern "C" {

int nastar_fields_grad_tiled_abi(void) { return NASTAR_FIELDS_GRAD_TILED_ABI; }

int nastar_fields_grad_tiled_max_cells(void) { return kGradTiledMaxCells; }

size_t nastar_fields_backward_tiled_workspace_bytes(int B, int H, int W)
{
    if (!tiled_shape_ok(B, H, W)) return 0;
    return ((size_t)B * H * W * 9 + (size_t)B * 16 + (size_t)B * (size_t)tile_count(H, W) * 8 + 15) / 16 * 16;
}

int nastar_fields_backward_tiled(const float* dist, const float* goal, const float* passable, const float* grad_dist, int B, int H, int W,
                                 unsigned neighbor_mask, float* grad_cost_out, int32_t* status_out, int32_t* visits_out, void* workspace,
                                 size_t workspace_bytes, long long max_rounds, int* rounds_out, void* stream)
{
    GradTiledArgs a;
    int rc = gtl_args(dist, goal, passable, grad_dist, true, B, H, W, neighbor_mask, grad_cost_out, status_out, visits_out, workspace, workspace_bytes,
                      max_rounds, &a);
    if (rc) return rc;
    const dim3 grid((unsigned)(B * tile_count(H, W)));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    rc = clear_map_words(a.words, B, s);
    if (rc) return rc;
    rc = launch_grid(nastar_fields_grad_tiled_init_kernel, grid, dim3(kTileT), 0, s, a);
    if (rc) return rc;
    const Rounds r = run_rounds(a.words, B, H, W, max_rounds, kGradTiledLaunchesPerBatch, s,
                                [&](int round) { return launch_grid(nastar_fields_grad_tiled_round_kernel, grid, dim3(kTileT), 0, s, a, round); });
    if (r.rc) return r.rc;
    rc = launch_grid(nastar_fields_grad_tiled_finish_kernel, grid, dim3(kTileT), 0, s, a, (int)r.launched);
    if (rc) return rc;
    if (rounds_out) *rounds_out = r.active_rounds;
    return NASTAR_OK;
}

int nastar_fields_backward_tiled_status(const float* dist, const float* goal, const float* passable, int B, int H, int W,
                                        unsigned neighbor_mask, int32_t* status_out, void* workspace, size_t workspace_bytes, void* stream)
{
    GradTiledArgs a;
    int rc = gtl_args(dist, goal, passable, nullptr, false, B, H, W, neighbor_mask, nullptr, status_out, nullptr, workspace, workspace_bytes, 0, &a);
    if (rc) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    rc = clear_map_words(a.words, B, s);
    if (rc) return rc;
    rc = launch_grid(nastar_fields_grad_tiled_init_kernel, dim3((unsigned)(B * tile_count(H, W))), dim3(kTileT), 0, s, a);
    if (rc) return rc;
    return launch_grid(nastar_fields_grad_tiled_status_kernel, dim3((unsigned)((B + kTileT - 1) / kTileT)), dim3(kTileT), 0, s, a);
}

}  // extern "C"
