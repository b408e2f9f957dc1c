// nastar_soft_fields_tiled_capi.hip -- the C ABI of include/nastar_soft_fields_tiled.h: the entropy-regularised cost-to-go field and its
// gradient by tiled sweeps, with a checkpointed tape.  A translation unit of its own: nothing here touches the other field kernels.  Both
// entry points only enqueue: nothing is read back.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>

#include "nastar_fields_host.hip.h"
#include "nastar_soft_fields_tiled.hip.h"

using namespace nastar;

static_assert(soft_tile_lds_bytes(kSoftTileSweeps) <= kMaxLdsBytes / 2, "two workgroups of the widest sweep launch share a CU's LDS");
static_assert(soft_tile_grad_lds_bytes() <= kMaxLdsBytes / 2, "... and two of a step launch");
static_assert((kTileH + 3) * (kTileW + 5) <= kSoftFieldsGradMaxCells, "a map with seams both ways and ragged last tiles fits the one-workgroup backward");
static_assert((2 * kTileH + 1) * (kTileW + 1) <= kSoftFieldsMaxCells, "a map with a tile between two others fits the one-workgroup forward");

namespace {

using u128 = unsigned __int128;

constexpr u128 pad(u128 n, unsigned to) { return (n + (to - 1)) / to * to; }
inline size_t fit(u128 n) { return n > (u128)SIZE_MAX ? SIZE_MAX : (size_t)n; }

// bytes of one plane of the batch ([B,HW] fp32), padded so that every plane of a workspace starts on a 16-byte boundary
inline u128 plane_bytes(int B, int H, int W) { return pad((u128)(unsigned)B * ((u128)(unsigned)H * (unsigned)W) * 4u, 16); }
inline u128 flag_bytes(int B) { return pad((u128)(unsigned)B * 8u, 256); }
inline int segment_planes(int horizon, int c) { return std::min(c, horizon) - 1; }

// the refusals both entry points share, behind their NULL checks: -> a status, NASTAR_OK to go on
int soft_tiled_call_ok(int B, int H, int W, double tau, int horizon, int c, int sweeps, const void* tape, size_t tape_bytes, const void* workspace,
                       size_t workspace_bytes, size_t workspace_needed)
{
    if (B < 1 || H < 1 || W < 1 || horizon < 1 || c < 1 || !(tau > 0.0) || !std::isfinite(tau)) return NASTAR_ERR_BAD_SHAPE;
    if (sweeps < 1 || sweeps > kSoftTileSweeps) return NASTAR_ERR_BAD_SHAPE;
    if (!tiled_shape_ok(B, H, W)) return NASTAR_ERR_UNSUPPORTED;   // above kTiledMaxCells cells, or more than 2^24 tiles in the batch
    if (tape && (tape_bytes < nastar_soft_fields_tiled_tape_bytes(B, H, W, horizon, c) || !aligned16(tape))) return NASTAR_ERR_WORKSPACE;
    if (workspace_bytes < workspace_needed || !aligned16(workspace)) return NASTAR_ERR_WORKSPACE;
    return NASTAR_OK;
}

struct Geometry {
    TileGrid g;
    unsigned tiles;       // of the batch
    size_t plane;         // floats from one plane of a workspace or a tape to the next
};
Geometry geometry(int B, int H, int W)
{
    const TileGrid g{B, H, W, tiles_down(H), tiles_across(W)};
    return {g, (unsigned)((long long)B * tile_count(H, W)), (size_t)B * ((size_t)H * W)};
}

int prepare(const float* cost, const float* goal, const float* passable, float* C, float* V0, int32_t* flags, int32_t* status, int B, int HW,
            bool report_no_goal, double tau, hipStream_t s)
{
    const SoftPrepareArgs a{cost, goal, passable, C, V0, flags, status, HW, report_no_goal ? 1 : 0, (float)(1.0 / (tau * M_LN2))};
    return launch_grid(nastar_soft_tiled_prepare_kernel<kSoftTileT>, dim3((unsigned)B), dim3(kSoftTileT), 0, s, a);
}

// one launch of a.n sweeps from plane a.k0 on every tile of the batch
int launch_sweeps(const SoftTileArgs& a, const Geometry& geo, hipStream_t s)
{
    return launch_grid(nastar_soft_tiled_sweeps_kernel<kSoftTileT>, dim3(geo.tiles), dim3(kSoftTileT), soft_tile_lds_bytes(a.n), s, a);
}

int forward(const float* cost, const float* goal, const float* passable, int B, int H, int W, unsigned neighbor_mask, double tau, int horizon,
            float* dist_out, float* policy_out, int32_t* status_out, void* tape, size_t tape_bytes, int c, void* workspace, size_t workspace_bytes,
            int sweeps, void* stream)
{
    if (!field_mask_ok(neighbor_mask)) return NASTAR_ERR_UNSUPPORTED;
    if (!cost || !goal || !passable || !dist_out || !status_out || !workspace) return NASTAR_ERR_NULL;
    if (int rc = soft_tiled_call_ok(B, H, W, tau, horizon, c, sweeps, tape, tape_bytes, workspace, workspace_bytes,
                                    nastar_soft_fields_tiled_workspace_bytes(B, H, W)))
        return rc;
    const Geometry geo = geometry(B, H, W);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    int32_t* flags = reinterpret_cast<int32_t*>(ws);
    float* C = reinterpret_cast<float*>(ws + (size_t)flag_bytes(B));
    const size_t stride = (size_t)plane_bytes(B, H, W) / 4;
    float* planes[2] = {C + stride, C + 2 * stride};
    if (int rc = prepare(cost, goal, passable, C, planes[0], flags, status_out, B, H * W, true, tau, s)) return rc;

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
    return fit(flag_bytes(B) + 3 * plane_bytes(B, H, W));
}

size_t nastar_soft_fields_tiled_tape_bytes(int B, int H, int W, int horizon, int checkpoint_every)
{
    if (B < 1 || H < 1 || W < 1 || horizon < 1 || checkpoint_every < 1) return 0;
    return fit((u128)(unsigned)B * ((u128)(unsigned)H * (unsigned)W) * 4u * ((u128)(unsigned)(horizon / checkpoint_every) + 1u));
}

size_t nastar_soft_fields_tiled_backward_workspace_bytes(int B, int H, int W, int horizon, int checkpoint_every)
{
    if (B < 1 || H < 1 || W < 1 || horizon < 1 || checkpoint_every < 1) return 0;
    // flags; C, V_0, A twice and the fp64 sums (two planes' worth); the segment buffer, planes of the tape's own stride
    return fit(flag_bytes(B) + 6 * plane_bytes(B, H, W)
               + (u128)(unsigned)segment_planes(horizon, checkpoint_every) * ((u128)(unsigned)B * ((u128)(unsigned)H * (unsigned)W) * 4u));
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
    const Geometry geo = geometry(B, H, W);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    int32_t* flags = reinterpret_cast<int32_t*>(ws);
    float* C = reinterpret_cast<float*>(ws + (size_t)flag_bytes(B));
    const size_t stride = (size_t)plane_bytes(B, H, W) / 4;
    float* V0 = C + stride;
    float* A[2] = {C + 2 * stride, C + 3 * stride};
    double* sum = reinterpret_cast<double*>(C + 4 * stride);
    float* seg = C + 6 * stride;                          // planes lo + 1, lo + 2, ... of the segment that starts behind plane lo
    const float* ck = static_cast<const float*>(tape);   // slot j - 1 is plane j * c; slot K / c is plane K
    const int n_ck = K / c;
    if (int rc = prepare(cost, goal, passable, C, V0, flags, status_out, B, H * W, false, tau, s)) return rc;

    // (the tape is in units of tau * ln 2 and the gradient with respect to the cost needs no factor)
    SoftTileGradArgs ga{C, ck + (size_t)n_ck * geo.plane, nullptr, A[0], sum, grad_dist, grad_cost_out, flags, geo.g, neighbor_mask};
    if (int rc = launch_grid(nastar_soft_tiled_grad_init_kernel<kSoftPlaneT>, dim3(geo.tiles), dim3(kSoftPlaneT), 0, s, ga)) return rc;

    SoftTileArgs fa{};
    fa.C = C;
    fa.tape = seg;
    fa.g = geo.g;
    fa.tape_every = 1;
    fa.tape_count = INT_MAX;
    fa.final_k = fa.final_slot = -1;
    fa.nmask = neighbor_mask;
    int cur = 0;
    for (int j = n_ck; j >= 0; --j) {
        const int lo = j * c, hi = K - lo > c ? lo + c : K;  // the steps lo < k <= hi read the planes lo .. hi - 1; step 1 is never walked
        if (lo >= K) continue;                               // (K is a multiple of c: nothing lies above the last checkpoint)
        const int bottom = std::max(lo + 1, 2);
        if (hi < bottom) continue;
        const float* first = lo == 0 ? V0 : ck + (size_t)(j - 1) * geo.plane;
        auto plane = [&](int k) -> const float* { return k == lo ? first : seg + (size_t)(k - lo - 1) * geo.plane; };
        fa.tape_k0 = lo;
        for (int k0 = lo; k0 < hi - 1; k0 += fa.n) {   // the planes lo + 1 .. hi - 1, every one kept: the next launch reads it there
            fa.k0 = k0;
            fa.n = std::min(kSoftTileSweeps, hi - 1 - k0);
            fa.src = plane(k0);
            if (int rc = launch_sweeps(fa, geo, s)) return rc;
        }
        for (int k = hi; k >= bottom; --k) {
            ga.U = plane(k - 1);
            ga.A_in = A[cur];
            ga.A_out = A[cur ^ 1];
            if (int rc = launch_grid(nastar_soft_tiled_grad_step_kernel<kSoftTileT>, dim3(geo.tiles), dim3(kSoftTileT), soft_tile_grad_lds_bytes(), s, ga))
                return rc;
            cur ^= 1;
        }
    }
    return launch_grid(nastar_soft_tiled_grad_store_kernel<kSoftPlaneT>, dim3(geo.tiles), dim3(kSoftPlaneT), 0, s, ga);
}

}  // extern "C"
