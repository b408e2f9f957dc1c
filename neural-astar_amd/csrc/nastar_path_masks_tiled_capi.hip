// nastar_path_masks_tiled_capi.hip -- the C ABI of include/nastar_path_masks_tiled.h: the exact shortest-path mask and its blackbox gradient
// for maps of up to 1179648 cells.  A translation unit of its own: the field comes from the library's own nastar_cost_to_go_tiled, called
// as any user calls it -- the relaxation kernels are not compiled here -- and nothing here touches the search, replay, encoder or the
// other field kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "nastar_fields_host.hip.h"
#include "nastar_path_masks_tiled.hip.h"

using namespace nastar;

// the workspace: [the perturbed costs, 4 B per cell (backward)] [the field, 4 B per cell] [the relaxation's per-map status, rounded up to 16
// bytes] [the relaxation's own workspace] [the successor table, 1 B per cell, rounded up to 4 bytes]
struct PathTiledSpace {
    float* perturbed;
    float* dist;
    int32_t* field_status;
    void* field_ws;
    size_t field_ws_bytes;
    uint8_t* table;
};

static size_t ptl_status_bytes(int B) { return ((size_t)B * 4 + 15) / 16 * 16; }

static size_t ptl_workspace_bytes(int B, int H, int W, bool backward)
{
    if (!tiled_shape_ok(B, H, W)) return 0;
    const size_t plane = (size_t)B * H * W * 4;
    return (backward ? 2 : 1) * plane + ptl_status_bytes(B) + nastar_cost_to_go_tiled_workspace_bytes(B, H, W) + (plane / 4 + 3) / 4 * 4;
}

static PathTiledSpace ptl_carve(void* workspace, int B, int H, int W, bool backward)
{
    const size_t plane = (size_t)B * H * W * 4;
    char* w = reinterpret_cast<char*>(workspace);
    PathTiledSpace s;
    s.perturbed = backward ? reinterpret_cast<float*>(w) : nullptr;
    if (backward) w += plane;
    s.dist = reinterpret_cast<float*>(w);
    s.field_status = reinterpret_cast<int32_t*>(w + plane);
    s.field_ws = w + plane + ptl_status_bytes(B);
    s.field_ws_bytes = nastar_cost_to_go_tiled_workspace_bytes(B, H, W);   // (a multiple of 16)
    s.table = reinterpret_cast<uint8_t*>(s.field_ws) + s.field_ws_bytes;
    return s;
}

// the refusals both calls share behind their NULL checks, in the header's order; `steps_ok`: the backward's lambda / min_cost check
static int ptl_refuse(int B, int H, int W, long long max_rounds, bool steps_ok, const void* workspace, size_t workspace_bytes, bool backward)
{
    if (B < 1 || H < 1 || W < 1 || max_rounds < 0) return NASTAR_ERR_BAD_SHAPE;
    if (!tiled_shape_ok(B, H, W)) return NASTAR_ERR_UNSUPPORTED;
    if (!steps_ok) return NASTAR_ERR_UNSUPPORTED;
    if (workspace_bytes < ptl_workspace_bytes(B, H, W, backward) || (reinterpret_cast<uintptr_t>(workspace) & 3u) != 0) return NASTAR_ERR_WORKSPACE;
    return NASTAR_OK;
}

// behind the relaxation: the successor table, then the rows -- a workgroup per map
template <bool kBackward>
static int ptl_mark(const PathMarkArgs& a, int B, hipStream_t s)
{
    const int groups = (a.H * a.W + kPathTableCells - 1) / kPathTableCells;   // (B * groups <= B * tiles <= 2^24)
    int rc = launch_grid(nastar_path_masks_tiled_table_kernel, dim3((unsigned)B * (unsigned)groups), dim3(kPathTableT), 0, s, a, groups);
    if (rc) return rc;
    return launch_grid(nastar_path_masks_tiled_mark_kernel<kBackward>, dim3((unsigned)B), dim3(kPathMarkT), 0, s, a);
}

extern "C" {

int nastar_path_masks_tiled_abi(void) { return NASTAR_PATH_MASKS_TILED_ABI; }

int nastar_path_masks_tiled_max_cells(void) { return kTiledMaxCells; }

size_t nastar_path_masks_tiled_workspace_bytes(int B, int H, int W) { return ptl_workspace_bytes(B, H, W, false); }

size_t nastar_path_masks_tiled_backward_workspace_bytes(int B, int H, int W) { return ptl_workspace_bytes(B, H, W, true); }

int nastar_path_masks_tiled(const float* cost, const float* goal, const float* passable, const int32_t* start_idx, int B, int H, int W,
                            unsigned neighbor_mask, float* path_out, float* path_cost_out, int32_t* status_out, void* workspace,
                            size_t workspace_bytes, long long max_rounds, int* rounds_out, void* stream)
{
    if (!field_mask_ok(neighbor_mask)) return NASTAR_ERR_UNSUPPORTED;
    if (!cost || !goal || !passable || !start_idx || !path_out || !status_out || !workspace) return NASTAR_ERR_NULL;
    int rc = ptl_refuse(B, H, W, max_rounds, true, workspace, workspace_bytes, false);
    if (rc) return rc;
    const PathTiledSpace w = ptl_carve(workspace, B, H, W, false);
    rc = nastar_cost_to_go_tiled(cost, goal, passable, B, H, W, neighbor_mask, w.dist, nullptr, w.field_status, nullptr, w.field_ws, w.field_ws_bytes,
                                 max_rounds, rounds_out, stream);
    if (rc) return rc;
    const PathMarkArgs a{w.dist, goal, passable, start_idx, w.field_status, w.table, nullptr, nullptr, path_out, path_cost_out, status_out, 0.f, H, W,
                         neighbor_mask};
    return ptl_mark<false>(a, B, reinterpret_cast<hipStream_t>(stream));
}

int nastar_path_masks_tiled_backward(const float* cost, const float* goal, const float* passable, const int32_t* start_idx,
                                     const float* grad_path, const float* path_fwd, const int32_t* status_fwd, int B, int H, int W,
                                     unsigned neighbor_mask, float lambda, float min_cost, float* grad_cost_out, int32_t* status_out,
                                     void* workspace, size_t workspace_bytes, long long max_rounds, int* rounds_out, void* stream)
{
    if (!field_mask_ok(neighbor_mask)) return NASTAR_ERR_UNSUPPORTED;
    if (!cost || !goal || !passable || !start_idx || !grad_path || !path_fwd || !status_fwd || !grad_cost_out || !workspace) return NASTAR_ERR_NULL;
    const float inv_lambda = lambda > 0.f ? 1.0f / lambda : 0.f;  // one IEEE fp32 division, on the host: what the kernel multiplies by
    const bool steps_ok = lambda > 0.f && std::isfinite(lambda) && min_cost > 0.f && std::isfinite(min_cost) && std::isfinite(inv_lambda);  // (a denormal lambda: 1 / lambda = inf)
    int rc = ptl_refuse(B, H, W, max_rounds, steps_ok, workspace, workspace_bytes, true);
    if (rc) return rc;
    const PathTiledSpace w = ptl_carve(workspace, B, H, W, true);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t cells = (size_t)B * H * W;
    const unsigned blocks = (unsigned)std::min<size_t>((cells + kPerturbT - 1) / kPerturbT, (size_t)1 << 20);
    rc = launch_grid(nastar_path_masks_tiled_perturb_kernel, dim3(blocks), dim3(kPerturbT), 0, s, cost, grad_path, w.perturbed, cells, lambda, min_cost);
    if (rc) return rc;
    rc = nastar_cost_to_go_tiled(w.perturbed, goal, passable, B, H, W, neighbor_mask, w.dist, nullptr, w.field_status, nullptr, w.field_ws,
                                 w.field_ws_bytes, max_rounds, rounds_out, stream);
    if (rc) return rc;
    const PathMarkArgs a{w.dist, goal, passable, start_idx, w.field_status, w.table, path_fwd, status_fwd, grad_cost_out, nullptr, status_out, inv_lambda,
                         H, W, neighbor_mask};
    return ptl_mark<true>(a, B, s);
}

}  // extern "C"
