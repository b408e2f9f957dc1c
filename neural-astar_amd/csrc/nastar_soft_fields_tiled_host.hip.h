// nastar_soft_fields_tiled_host.hip.h -- what the host sides of the tiled soft-field translation units share
// (nastar_soft_fields_tiled_capi.hip, nastar_soft_policy_tiled_capi.hip): the sizes, the refusals behind the NULL checks, the prepare
// launch, and the two drivers -- the forward's launches of sweeps and the backward's walk over the checkpointed tape -- with the launches
// that differ between the two handed in by the caller.  No kernel is instantiated here: each translation unit instantiates its own only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>

#include "nastar_fields_host.hip.h"
#include "nastar_soft_fields_tiled.hip.h"

namespace nastar {

using u128 = unsigned __int128;

constexpr u128 sft_pad(u128 n, unsigned to) { return (n + (to - 1)) / to * to; }
inline size_t sft_fit(u128 n) { return n > (u128)SIZE_MAX ? SIZE_MAX : (size_t)n; }

// bytes of one plane of the batch ([B,HW] fp32), padded so that every plane of a workspace starts on a 16-byte boundary
inline u128 sft_plane_bytes(int B, int H, int W) { return sft_pad((u128)(unsigned)B * ((u128)(unsigned)H * (unsigned)W) * 4u, 16); }
inline u128 sft_flag_bytes(int B) { return sft_pad((u128)(unsigned)B * 8u, 256); }
inline int sft_segment_planes(int horizon, int c) { return std::min(c, horizon) - 1; }

// the refusals the entry points share, behind their NULL checks: -> a status, NASTAR_OK to go on
inline int soft_tiled_call_ok(int B, int H, int W, double tau, int horizon, int c, int sweeps, const void* tape, size_t tape_bytes,
                              const void* workspace, size_t workspace_bytes, size_t workspace_needed)
{
    if (B < 1 || H < 1 || W < 1 || horizon < 1 || c < 1 || !(tau > 0.0) || !std::isfinite(tau)) return NASTAR_ERR_BAD_SHAPE;
    if (sweeps < 1 || sweeps > kSoftTileSweeps) return NASTAR_ERR_BAD_SHAPE;
    if (!tiled_shape_ok(B, H, W)) return NASTAR_ERR_UNSUPPORTED;   // above kTiledMaxCells cells, or more than 2^24 tiles in the batch
    if (tape && (tape_bytes < nastar_soft_fields_tiled_tape_bytes(B, H, W, horizon, c) || !aligned16(tape))) return NASTAR_ERR_WORKSPACE;
    if (workspace_bytes < workspace_needed || !aligned16(workspace)) return NASTAR_ERR_WORKSPACE;
    return NASTAR_OK;
}

struct SoftTiledGeometry {
    TileGrid g;
    unsigned tiles;       // of the batch
    size_t plane;         // floats from one plane of a workspace or a tape to the next
};
inline SoftTiledGeometry soft_tiled_geometry(int B, int H, int W)
{
    const TileGrid g{B, H, W, tiles_down(H), tiles_across(W)};
    return {g, (unsigned)((long long)B * tile_count(H, W)), (size_t)B * ((size_t)H * W)};
}

// The launches of the plain kernels, defined in nastar_soft_fields_tiled_capi.hip: the one translation unit that instantiates them.
int soft_tiled_prepare(const float* cost, const float* goal, const float* passable, float* C, float* V0, int32_t* flags, int32_t* status, int B,
                       int HW, bool report_no_goal, double tau, hipStream_t s);
// one launch of a.n sweeps from plane a.k0 on every tile of the batch
int soft_tiled_launch_sweeps(const SoftTileArgs& a, const SoftTiledGeometry& geo, hipStream_t s);
int soft_tiled_launch_init(const SoftTileGradArgs& ga, const SoftTiledGeometry& geo, hipStream_t s);
int soft_tiled_launch_step(const SoftTileGradArgs& ga, const SoftTiledGeometry& geo, hipStream_t s);
int soft_tiled_launch_store(const SoftTileGradArgs& ga, const SoftTiledGeometry& geo, hipStream_t s);

// THE FORWARD behind its refusals: the prepare launch, then ceil(horizon / sweeps) launches through launch_sweeps(a, geo, s) -> a status
// (a.last says which one reaches the horizon)
template <typename LaunchSweeps>
inline int soft_tiled_forward(const float* cost, const float* goal, const float* passable, int B, int H, int W, unsigned neighbor_mask, double tau,
                              int horizon, float* dist_out, float* policy_out, int32_t* status_out, void* tape, int c, void* workspace, int sweeps,
                              void* stream, LaunchSweeps&& launch_sweeps)
{
    const SoftTiledGeometry geo = soft_tiled_geometry(B, H, W);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    int32_t* flags = reinterpret_cast<int32_t*>(ws);
    float* C = reinterpret_cast<float*>(ws + (size_t)sft_flag_bytes(B));
    const size_t stride = (size_t)sft_plane_bytes(B, H, W) / 4;
    float* planes[2] = {C + stride, C + 2 * stride};
    if (int rc = soft_tiled_prepare(cost, goal, passable, C, planes[0], flags, status_out, B, H * W, true, tau, s)) return rc;

    SoftTileArgs a{};
    a.C = C;
    a.tape = static_cast<float*>(tape);
    a.goal = goal;
    a.flags = flags;
    a.dist = dist_out;
    a.policy = policy_out;
    a.g = geo.g;
    a.tape_k0 = 0;
    a.tape_every = c;
    a.tape_count = horizon / c;
    a.final_k = horizon;
    a.final_slot = horizon / c;
    a.nmask = neighbor_mask;
    a.from_units = (float)(tau * M_LN2);
    // the launches ping-pong between the two planes; the one that reaches the horizon stores dist (and the tape's last slot) instead
    float *src = planes[0], *dst = planes[1];
    for (int k0 = 0; k0 < horizon; k0 += a.n) {
        a.k0 = k0;
        a.n = std::min(sweeps, horizon - k0);
        a.last = k0 + a.n == horizon;
        a.src = src;
        a.dst = a.last ? nullptr : dst;
        if (int rc = launch_sweeps(a, geo, s)) return rc;
        std::swap(src, dst);
    }
    return NASTAR_OK;
}

// THE SEGMENTS of a checkpointed tape, top down: what the backward and the walkers of nastar_soft_routes_tiled_capi.hip share.  `ck` is the
// tape (slot j - 1 is plane j * c; slot K / c is plane K), V0 and C the prepare launch's planes, `seg` a buffer of sft_segment_planes(K, c)
// planes of the tape's stride.  For every segment, the steps lo < k <= hi that read the planes lo .. hi - 1, from the top: the sweeps that
// rebuild the planes lo + 1 .. hi - 1 from plane lo into `seg`, then visit(lo, hi, bottom, plane) -> a status, with plane(k) the plane
// lo <= k < hi and `bottom` = max(lo + 1, lowest) the lowest step the caller walks (a segment wholly below `lowest` is skipped).
template <typename Visit>
inline int soft_tiled_each_segment(const float* C, const float* V0, const float* ck, float* seg, int K, int c, int lowest, unsigned neighbor_mask,
                                   const SoftTiledGeometry& geo, hipStream_t s, Visit&& visit)
{
    SoftTileArgs fa{};
    fa.C = C;
    fa.tape = seg;
    fa.g = geo.g;
    fa.tape_every = 1;
    fa.tape_count = INT_MAX;
    fa.final_k = fa.final_slot = -1;
    fa.nmask = neighbor_mask;
    for (int j = K / c; j >= 0; --j) {
        const int lo = j * c, hi = K - lo > c ? lo + c : K;
        if (lo >= K) continue;                               // (K is a multiple of c: nothing lies above the last checkpoint)
        const int bottom = std::max(lo + 1, lowest);
        if (hi < bottom) continue;
        const float* first = lo == 0 ? V0 : ck + (size_t)(j - 1) * geo.plane;
        auto plane = [&](int k) -> const float* { return k == lo ? first : seg + (size_t)(k - lo - 1) * geo.plane; };
        fa.tape_k0 = lo;
        for (int k0 = lo; k0 < hi - 1; k0 += fa.n) {   // the planes lo + 1 .. hi - 1, every one kept: the next launch reads it there
            fa.k0 = k0;
            fa.n = std::min(kSoftTileSweeps, hi - 1 - k0);
            fa.src = plane(k0);
            if (int rc = soft_tiled_launch_sweeps(fa, geo, s)) return rc;
        }
        if (int rc = visit(lo, hi, bottom, plane)) return rc;
    }
    return NASTAR_OK;
}

// THE BACKWARD behind its refusals: prepare, launch_init(ga, geo, s) for A_K and the sums, then segment by segment, top down, the sweeps
// that rebuild the segment's planes and launch_step(ga, k, plane_K, geo, s) for k = K .. 2 (ga.U is plane k - 1), and the store launch
template <typename LaunchInit, typename LaunchStep>
inline int soft_tiled_backward(const float* cost, const float* goal, const float* passable, const void* tape, int c, const float* grad_dist, int B,
                               int H, int W, unsigned neighbor_mask, double tau, int K, float* grad_cost_out, int32_t* status_out, void* workspace,
                               void* stream, LaunchInit&& launch_init, LaunchStep&& launch_step)
{
    const SoftTiledGeometry geo = soft_tiled_geometry(B, H, W);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    int32_t* flags = reinterpret_cast<int32_t*>(ws);
    float* C = reinterpret_cast<float*>(ws + (size_t)sft_flag_bytes(B));
    const size_t stride = (size_t)sft_plane_bytes(B, H, W) / 4;
    float* V0 = C + stride;
    float* A[2] = {C + 2 * stride, C + 3 * stride};
    double* sum = reinterpret_cast<double*>(C + 4 * stride);
    float* seg = C + 6 * stride;                          // planes lo + 1, lo + 2, ... of the segment that starts behind plane lo
    const float* ck = static_cast<const float*>(tape);   // slot j - 1 is plane j * c; slot K / c is plane K
    const float* plane_K = ck + (size_t)(K / c) * geo.plane;
    if (int rc = soft_tiled_prepare(cost, goal, passable, C, V0, flags, status_out, B, H * W, false, tau, s)) return rc;

    // (the tape is in units of tau * ln 2 and the gradient with respect to the cost needs no factor)
    SoftTileGradArgs ga{C, plane_K, nullptr, A[0], sum, grad_dist, grad_cost_out, flags, geo.g, neighbor_mask};
    if (int rc = launch_init(ga, geo, s)) return rc;

    int cur = 0;  // (step 1 is never walked: lowest = 2)
    const int rc = soft_tiled_each_segment(C, V0, ck, seg, K, c, 2, neighbor_mask, geo, s, [&](int, int hi, int bottom, auto&& plane) {
        for (int k = hi; k >= bottom; --k) {
            ga.U = plane(k - 1);
            ga.A_in = A[cur];
            ga.A_out = A[cur ^ 1];
            if (int rc = launch_step(ga, k, plane_K, geo, s)) return rc;
            cur ^= 1;
        }
        return (int)NASTAR_OK;
    });
    if (rc) return rc;
    return soft_tiled_launch_store(ga, geo, s);
}

}  // namespace nastar
