// nastar_soft_policy_tiled_capi.hip -- the C ABI of include/nastar_soft_policy_tiled.h: the log-policy of the tiled entropy-regularised
// cost-to-go field and the gradient through it.  A translation unit of its own: it instantiates the log-policy epilogue, the NULL-tolerant
// init and the injected step; every other launch is nastar_soft_fields_tiled_capi.hip's.  Both entry points only enqueue.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "nastar_soft_fields_tiled_host.hip.h"
#include "nastar_soft_policy_tiled.hip.h"

using namespace nastar;

static_assert(soft_tile_inject_lds_bytes() <= kMaxLdsBytes / 2, "two workgroups of the injected step share a CU's LDS");

namespace {

int forward(const float* cost, const float* goal, const float* passable, int B, int H, int W, unsigned neighbor_mask, double tau, int horizon,
            float* dist_out, float* policy_out, float* log_policy_out, int32_t* status_out, void* tape, size_t tape_bytes, int c, void* workspace,
            size_t workspace_bytes, int sweeps, void* stream)
{
    if (!field_mask_ok(neighbor_mask)) return NASTAR_ERR_UNSUPPORTED;
    if (!cost || !goal || !passable || !dist_out || !log_policy_out || !status_out || !workspace) return NASTAR_ERR_NULL;
    if (int rc = soft_tiled_call_ok(B, H, W, tau, horizon, c, sweeps, tape, tape_bytes, workspace, workspace_bytes,
                                    nastar_soft_fields_tiled_workspace_bytes(B, H, W)))
        return rc;
    // the launch that reaches plane K is the one with the log-policy epilogue; the others are the plain kernel
    return soft_tiled_forward(cost, goal, passable, B, H, W, neighbor_mask, tau, horizon, dist_out, policy_out, status_out, tape, c, workspace, sweeps,
                              stream, [&](const SoftTileArgs& a, const SoftTiledGeometry& geo, hipStream_t s) {
                                  if (!a.last) return soft_tiled_launch_sweeps(a, geo, s);
                                  return launch_grid(nastar_soft_policy_tiled_sweeps_kernel<kSoftTileT>, dim3(geo.tiles), dim3(kSoftTileT),
                                                     soft_tile_lds_bytes(a.n), s, a, log_policy_out);
                              });
}

}  // namespace

extern "C" {

int nastar_soft_policy_tiled_abi(void) { return NASTAR_SOFT_POLICY_TILED_ABI; }

size_t nastar_soft_policy_tiled_backward_workspace_bytes(int B, int H, int W, int horizon, int checkpoint_every)
{
    return nastar_soft_fields_tiled_backward_workspace_bytes(B, H, W, horizon, checkpoint_every);  // (Q and the live bytes stay in LDS)
}

int nastar_soft_policy_forward_tiled(const float* cost, const float* goal, const float* passable, int B, int H, int W, unsigned neighbor_mask,
                                     double tau, int horizon, float* dist_out, float* policy_out, float* log_policy_out, int32_t* status_out,
                                     void* tape, size_t tape_bytes, int checkpoint_every, void* workspace, size_t workspace_bytes, void* stream)
{
    return forward(cost, goal, passable, B, H, W, neighbor_mask, tau, horizon, dist_out, policy_out, log_policy_out, status_out, tape, tape_bytes,
                   checkpoint_every, workspace, workspace_bytes, kSoftTileSweeps, stream);
}

int nastar_soft_policy_forward_tiled_with_sweeps(const float* cost, const float* goal, const float* passable, int B, int H, int W,
                                                 unsigned neighbor_mask, double tau, int horizon, float* dist_out, float* policy_out,
                                                 float* log_policy_out, int32_t* status_out, void* tape, size_t tape_bytes,
                                                 int checkpoint_every, void* workspace, size_t workspace_bytes, int sweeps_per_launch,
                                                 void* stream)
{
    return forward(cost, goal, passable, B, H, W, neighbor_mask, tau, horizon, dist_out, policy_out, log_policy_out, status_out, tape, tape_bytes,
                   checkpoint_every, workspace, workspace_bytes, sweeps_per_launch, stream);
}

int nastar_soft_policy_backward_tiled(const float* cost, const float* goal, const float* passable, const void* tape, size_t tape_bytes,
                                      int checkpoint_every, const float* grad_dist, const float* grad_log_policy, int B, int H, int W,
                                      unsigned neighbor_mask, double tau, int horizon, float* grad_cost_out, int32_t* status_out,
                                      void* workspace, size_t workspace_bytes, void* stream)
{
    const int c = checkpoint_every, K = horizon;
    if (!field_mask_ok(neighbor_mask)) return NASTAR_ERR_UNSUPPORTED;
    if (!cost || !goal || !passable || !tape || !grad_cost_out || !status_out || !workspace) return NASTAR_ERR_NULL;
    if (int rc = soft_tiled_call_ok(B, H, W, tau, K, c, 1, tape, tape_bytes, workspace, workspace_bytes,
                                    nastar_soft_policy_tiled_backward_workspace_bytes(B, H, W, K, c)))
        return rc;
    // (the log-policy is a plane's difference OVER tau; step K is the first step the walk launches, and the only one that injects)
    const float neg_inv_tau = (float)(-1.0 / tau);
    return soft_tiled_backward(
        cost, goal, passable, tape, c, grad_dist, B, H, W, neighbor_mask, tau, K, grad_cost_out, status_out, workspace, stream,
        [](const SoftTileGradArgs& ga, const SoftTiledGeometry& geo, hipStream_t s) {
            if (ga.grad_dist) return soft_tiled_launch_init(ga, geo, s);
            return launch_grid(nastar_soft_policy_tiled_grad_init_kernel<kSoftPlaneT>, dim3(geo.tiles), dim3(kSoftPlaneT), 0, s, ga);
        },
        [&](const SoftTileGradArgs& ga, int k, const float* plane_K, const SoftTiledGeometry& geo, hipStream_t s) {
            if (!grad_log_policy || k != K) return soft_tiled_launch_step(ga, geo, s);
            const SoftTilePolicySeed seed{grad_log_policy, plane_K, neg_inv_tau};
            return launch_grid(nastar_soft_policy_tiled_inject_step_kernel<kSoftTileT>, dim3(geo.tiles), dim3(kSoftTileT),
                               soft_tile_inject_lds_bytes(), s, ga, seed);
        });
}

}  // extern "C"
