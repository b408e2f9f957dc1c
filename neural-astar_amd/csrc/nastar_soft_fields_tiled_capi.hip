// nastar_soft_fields_tiled_capi.hip -- the C ABI of include/nastar_soft_fields_tiled.h: the entropy-regularised cost-to-go field and its
// gradient by tiled sweeps, with a checkpointed tape.  A translation unit of its own: nothing here touches the other field kernels.  Both
// entry points only enqueue: nothing is read back.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "nastar_soft_fields_tiled_host.hip.h"

using namespace nastar;

static_assert(soft_tile_lds_bytes(kSoftTileSweeps) <= kMaxLdsBytes / 2, "two workgroups of the widest sweep launch share a CU's LDS");
static_assert(soft_tile_grad_lds_bytes() <= kMaxLdsBytes / 2, "... and two of a step launch");
static_assert((kTileH + 3) * (kTileW + 5) <= kSoftFieldsGradMaxCells, "a map with seams both ways and ragged last tiles fits the one-workgroup backward");
static_assert((2 * kTileH + 1) * (kTileW + 1) <= kSoftFieldsMaxCells, "a map with a tile between two others fits the one-workgroup forward");

// the launches of the plain kernels (nastar_soft_fields_tiled_host.hip.h): this translation unit alone instantiates them
namespace nastar {

int soft_tiled_prepare(const float* cost, const float* goal, const float* passable, float* C, float* V0, int32_t* flags, int32_t* status, int B,
                       int HW, bool report_no_goal, double tau, hipStream_t s)
{
    const SoftPrepareArgs a{cost, goal, passable, C, V0, flags, status, HW, report_no_goal ? 1 : 0, (float)(1.0 / (tau * M_LN2))};
    return launch_grid(nastar_soft_tiled_prepare_kernel<kSoftTileT>, dim3((unsigned)B), dim3(kSoftTileT), 0, s, a);
}

int soft_tiled_launch_sweeps(const SoftTileArgs& a, const SoftTiledGeometry& geo, hipStream_t s)
{
    return launch_grid(nastar_soft_tiled_sweeps_kernel<kSoftTileT>, dim3(geo.tiles), dim3(kSoftTileT), soft_tile_lds_bytes(a.n), s, a, (float*)nullptr);
}

int soft_tiled_launch_init(const SoftTileGradArgs& ga, const SoftTiledGeometry& geo, hipStream_t s)
{
    return launch_grid(nastar_soft_tiled_grad_init_kernel<kSoftPlaneT>, dim3(geo.tiles), dim3(kSoftPlaneT), 0, s, ga);
}

int soft_tiled_launch_step(const SoftTileGradArgs& ga, const SoftTiledGeometry& geo, hipStream_t s)
{
    return launch_grid(nastar_soft_tiled_grad_step_kernel<kSoftTileT>, dim3(geo.tiles), dim3(kSoftTileT), soft_tile_grad_lds_bytes(), s, ga, SoftTilePolicySeed{nullptr, nullptr, 0.f});
}

int soft_tiled_launch_store(const SoftTileGradArgs& ga, const SoftTiledGeometry& geo, hipStream_t s)
{
    return launch_grid(nastar_soft_tiled_grad_store_kernel<kSoftPlaneT>, dim3(geo.tiles), dim3(kSoftPlaneT), 0, s, ga);
}

}  // namespace nastar

namespace {

int forward(const float* cost, const float* goal, const float* passable, int B, int H, int W, unsigned neighbor_mask, double tau, int horizon,
            float* dist_out, float* policy_out, int32_t* status_out, void* tape, size_t tape_bytes, int c, void* workspace, size_t workspace_bytes,
            int sweeps, void* stream)
{
    if (!field_mask_ok(neighbor_mask)) return NASTAR_ERR_UNSUPPORTED;
    if (!cost || !goal || !passable || !dist_out || !status_out || !workspace) return NASTAR_ERR_NULL;
    if (int rc = soft_tiled_call_ok(B, H, W, tau, horizon, c, sweeps, tape, tape_bytes, workspace, workspace_bytes,
                                    nastar_soft_fields_tiled_workspace_bytes(B, H, W)))
        return rc;
    return soft_tiled_forward(cost, goal, passable, B, H, W, neighbor_mask, tau, horizon, dist_out, policy_out, status_out, tape, c, workspace, sweeps,
                              stream, soft_tiled_launch_sweeps);
}

}  // namespace

extern "C" {

int nastar_soft_fields_tiled_abi(void) { return NASTAR_SOFT_FIELDS_TILED_ABI; }

int nastar_soft_fields_tiled_max_cells(void) { return kTiledMaxCells; }

int nastar_soft_fields_tile(int* th, int* tw, int* sweeps)
{
    if (th) *th = kTileH;
    if (tw) *tw = kTileW;
    if (sweeps) *sweeps = kSoftTileSweeps;
    return 0;
}

size_t nastar_soft_fields_tiled_workspace_bytes(int B, int H, int W)
{
    if (B < 1 || H < 1 || W < 1) return 0;
    return sft_fit(sft_flag_bytes(B) + 3 * sft_plane_bytes(B, H, W));
}

size_t nastar_soft_fields_tiled_tape_bytes(int B, int H, int W, int horizon, int checkpoint_every)
{
    if (B < 1 || H < 1 || W < 1 || horizon < 1 || checkpoint_every < 1) return 0;
    return sft_fit((u128)(unsigned)B * ((u128)(unsigned)H * (unsigned)W) * 4u * ((u128)(unsigned)(horizon / checkpoint_every) + 1u));
}

size_t nastar_soft_fields_tiled_backward_workspace_bytes(int B, int H, int W, int horizon, int checkpoint_every)
{
    if (B < 1 || H < 1 || W < 1 || horizon < 1 || checkpoint_every < 1) return 0;
    // flags; C, V_0, A twice and the fp64 sums (two planes' worth); the segment buffer, planes of the tape's own stride
    return sft_fit(sft_flag_bytes(B) + 6 * sft_plane_bytes(B, H, W)
               + (u128)(unsigned)sft_segment_planes(horizon, checkpoint_every) * ((u128)(unsigned)B * ((u128)(unsigned)H * (unsigned)W) * 4u));
}

int nastar_soft_cost_to_go_tiled(const float* cost, const float* goal, const float* passable, int B, int H, int W, unsigned neighbor_mask,
                                 double tau, int horizon, float* dist_out, float* policy_out, int32_t* status_out, void* tape,
                                 size_t tape_bytes, int checkpoint_every, void* workspace, size_t workspace_bytes, void* stream)
{
    return forward(cost, goal, passable, B, H, W, neighbor_mask, tau, horizon, dist_out, policy_out, status_out, tape, tape_bytes, checkpoint_every,
                   workspace, workspace_bytes, kSoftTileSweeps, stream);
}

int nastar_soft_cost_to_go_tiled_with_sweeps(const float* cost, const float* goal, const float* passable, int B, int H, int W,
                                             unsigned neighbor_mask, double tau, int horizon, float* dist_out, float* policy_out,
                                             int32_t* status_out, void* tape, size_t tape_bytes, int checkpoint_every, void* workspace,
                                             size_t workspace_bytes, int sweeps_per_launch, void* stream)
{
    return forward(cost, goal, passable, B, H, W, neighbor_mask, tau, horizon, dist_out, policy_out, status_out, tape, tape_bytes, checkpoint_every,
                   workspace, workspace_bytes, sweeps_per_launch, stream);
}

int nastar_soft_fields_backward_tiled(const float* cost, const float* goal, const float* passable, const void* tape, size_t tape_bytes,
                                      int checkpoint_every, const float* grad_dist, int B, int H, int W, unsigned neighbor_mask, double tau,
                                      int horizon, float* grad_cost_out, int32_t* status_out, void* workspace, size_t workspace_bytes,
                                      void* stream)
{
    const int c = checkpoint_every, K = horizon;
    if (!field_mask_ok(neighbor_mask)) return NASTAR_ERR_UNSUPPORTED;
    if (!cost || !goal || !passable || !tape || !grad_dist || !grad_cost_out || !status_out || !workspace) return NASTAR_ERR_NULL;
    if (int rc = soft_tiled_call_ok(B, H, W, tau, K, c, 1, tape, tape_bytes, workspace, workspace_bytes,
                                    nastar_soft_fields_tiled_backward_workspace_bytes(B, H, W, K, c)))
        return rc;
    return soft_tiled_backward(cost, goal, passable, tape, c, grad_dist, B, H, W, neighbor_mask, tau, K, grad_cost_out, status_out, workspace, stream,
                               soft_tiled_launch_init,
                               [](const SoftTileGradArgs& ga, int, const float*, const SoftTiledGeometry& geo, hipStream_t s) {
                                   return soft_tiled_launch_step(ga, geo, s);
                               });
}

}  // extern "C"
