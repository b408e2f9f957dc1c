// nastar_fields_grad_tiled_capi.hip -- the C ABI of include/nastar_fields_grad_tiled.h: the gradient of the cost-to-go field with respect to
// the cost maps for maps of up to 1179648 cells, by a tiled subtree sum.  A translation unit of its own: nothing here touches the search,
// replay, encoder, forward field or one-workgroup gradient kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "nastar_fields_grad_tiled.hip.h"
#include "nastar_host.hip.h"

using namespace nastar;

// rounds enqueued between two reads of the host: the forward's choice (nastar_fields_tiled_capi.hip)
constexpr int kGradTiledLaunchesPerBatch = 8;

static inline long long gtl_tiles(int H, int W) { return (long long)((H + kTileH - 1) / kTileH) * ((W + kTileW - 1) / kTileW); }

static inline bool gtl_shape_ok(int B, int H, int W)
{
    return B >= 1 && H >= 1 && W >= 1 && (long long)H * W <= kGradTiledMaxCells && (long long)B * gtl_tiles(H, W) <= (1ll << 24);   // (x 256 lanes: the 2^32 threads a grid may have)
}

// the refusals both entry points share, in the header's order, and the arguments of the kernels
static int gtl_args(const float* dist, const float* goal, const float* passable, const float* grad_dist, bool want_grad, int B, int H, int W,
                    unsigned neighbor_mask, float* grad_cost_out, int32_t* status_out, int32_t* visits_out, void* workspace, size_t workspace_bytes,
                    long long max_rounds, GradTiledArgs* out)
{
    if ((neighbor_mask & ~0x1FFu) != 0u || (neighbor_mask & 0x10u) != 0u) return NASTAR_ERR_UNSUPPORTED;
    if (!dist || !goal || !passable || !status_out || !workspace || (want_grad && (!grad_dist || !grad_cost_out))) return NASTAR_ERR_NULL;
    if (B < 1 || H < 1 || W < 1 || max_rounds < 0) return NASTAR_ERR_BAD_SHAPE;
    if (!gtl_shape_ok(B, H, W)) return NASTAR_ERR_UNSUPPORTED;
    if (workspace_bytes < nastar_fields_backward_tiled_workspace_bytes(B, H, W) || (reinterpret_cast<uintptr_t>(workspace) & 7u) != 0) return NASTAR_ERR_WORKSPACE;
    // A first (8-byte words), then the four per-map words (a block of B x 16 bytes, zeroed by one memset), the two flag arrays, the successor bytes
    const size_t cells = (size_t)B * H * W, tiles = (size_t)B * (size_t)gtl_tiles(H, W);
    char* w = reinterpret_cast<char*>(workspace);
    double* acc = reinterpret_cast<double*>(w);
    int32_t* words = reinterpret_cast<int32_t*>(w + cells * 8);
    int32_t* flags = words + (size_t)B * 4;
    uint8_t* succ = reinterpret_cast<uint8_t*>(flags + tiles * 2);
    *out = GradTiledArgs{dist, goal, passable, grad_dist, grad_cost_out, status_out, visits_out, acc, succ, words, flags,
                         B, H, W, (H + kTileH - 1) / kTileH, (W + kTileW - 1) / kTileW, neighbor_mask};
    return NASTAR_OK;
}

extern "C" {

int nastar_fields_grad_tiled_abi(void) { return NASTAR_FIELDS_GRAD_TILED_ABI; }

int nastar_fields_grad_tiled_max_cells(void) { return kGradTiledMaxCells; }

size_t nastar_fields_backward_tiled_workspace_bytes(int B, int H, int W)
{
    if (!gtl_shape_ok(B, H, W)) return 0;
    return ((size_t)B * H * W * 9 + (size_t)B * 16 + (size_t)B * (size_t)gtl_tiles(H, W) * 8 + 15) / 16 * 16;
}

int nastar_fields_backward_tiled(const float* dist, const float* goal, const float* passable, const float* grad_dist, int B, int H, int W,
                                 unsigned neighbor_mask, float* grad_cost_out, int32_t* status_out, int32_t* visits_out, void* workspace,
                                 size_t workspace_bytes, long long max_rounds, int* rounds_out, void* stream)
{
    GradTiledArgs a;
    int rc = gtl_args(dist, goal, passable, grad_dist, true, B, H, W, neighbor_mask, grad_cost_out, status_out, visits_out, workspace, workspace_bytes,
                      max_rounds, &a);
    if (rc) return rc;
    const dim3 grid((unsigned)((long long)B * a.ty * a.tx));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long bound = (long long)H * W + 1;  // every round with an active tile makes one more cell final
    const long long limit = max_rounds == 0 ? bound : std::min(max_rounds, bound);

    hipError_t e = hipMemsetAsync(a.words, 0, (size_t)B * 16, s);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(per-map words)");
    rc = launch_grid(nastar_fields_grad_tiled_init_kernel, grid, dim3(kTileT), 0, s, a);
    if (rc) return rc;

    // words[0..B): the last round in which the map marked a tile; words[B..2B): the last round in which it recomputed one
    std::vector<int32_t> host((size_t)B * 2);
    long long launched = 0;
    int active_rounds = 0;
    bool quiet = false;
    while (!quiet && launched < limit) {
        const long long n = std::min((long long)kGradTiledLaunchesPerBatch, limit - launched);
        for (long long k = 0; k < n; ++k) {
            rc = launch_grid(nastar_fields_grad_tiled_round_kernel, grid, dim3(kTileT), 0, s, a, (int)(launched + 1));
            if (rc) return rc;
            ++launched;
        }
        e = hipMemcpyAsync(host.data(), a.words, host.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(per-map words)");
        e = hipStreamSynchronize(s);
        if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
        quiet = *std::max_element(host.begin(), host.begin() + B) < launched;   // nobody marked a tile in the batch's last round
        active_rounds = *std::max_element(host.begin() + B, host.end());
    }
    rc = launch_grid(nastar_fields_grad_tiled_finish_kernel, grid, dim3(kTileT), 0, s, a, (int)launched);
    if (rc) return rc;
    if (rounds_out) *rounds_out = active_rounds;
    return NASTAR_OK;
}

int nastar_fields_backward_tiled_status(const float* dist, const float* goal, const float* passable, int B, int H, int W,
                                        unsigned neighbor_mask, int32_t* status_out, void* workspace, size_t workspace_bytes, void* stream)
{
    GradTiledArgs a;
    int rc = gtl_args(dist, goal, passable, nullptr, false, B, H, W, neighbor_mask, nullptr, status_out, nullptr, workspace, workspace_bytes, 0, &a);
    if (rc) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(a.words, 0, (size_t)B * 16, s);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(per-map words)");
    rc = launch_grid(nastar_fields_grad_tiled_init_kernel, dim3((unsigned)((long long)B * a.ty * a.tx)), dim3(kTileT), 0, s, a);
    if (rc) return rc;
    return launch_grid(nastar_fields_grad_tiled_status_kernel, dim3((unsigned)((B + kTileT - 1) / kTileT)), dim3(kTileT), 0, s, a);
}

}  // extern "C"
