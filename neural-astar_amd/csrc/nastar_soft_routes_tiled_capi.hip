// nastar_soft_routes_tiled_capi.hip -- the C ABI of include/nastar_soft_routes_tiled.h: sampled routes from the maximum-entropy route
// distribution, read from the tiled soft field's checkpointed tape.  A translation unit of its own: it instantiates the walker kernel and
// nothing else -- the prepare and sweep launches are nastar_soft_fields_tiled_capi.hip's, the clear launch nastar_soft_routes_capi.hip's.
// The call only enqueues: nothing is read back.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "nastar_soft_fields_tiled_host.hip.h"
#include "nastar_soft_routes_tiled.hip.h"

using namespace nastar;

namespace {

constexpr long long kSoftRoutesTiledMaxWalkers = 1ll << 30;

// the workspace: the flags and the prepare launch's per-map status, C, V_0, the walkers' state, the segment buffer -- every part starts
// on a 16-byte boundary
u128 state_bytes(int B, int S, int N) { return (u128)(unsigned)B * ((u128)(unsigned)S * (unsigned)N) * sizeof(SoftRoutesTiledState); }
u128 workspace_needed(int B, int S, int N, int H, int W, int K, int c)
{
    return 2 * sft_flag_bytes(B) + 2 * sft_plane_bytes(B, H, W) + state_bytes(B, S, N)
         + (u128)(unsigned)sft_segment_planes(K, c) * ((u128)(unsigned)B * ((u128)(unsigned)H * (unsigned)W) * 4u);
}

}  // namespace

extern "C" {

int nastar_soft_routes_tiled_abi(void) { return NASTAR_SOFT_ROUTES_TILED_ABI; }

int nastar_soft_routes_tiled_max_cells(void) { return kTiledMaxCells; }

size_t nastar_soft_routes_tiled_workspace_bytes(int B, int S, int N, int H, int W, int horizon, int checkpoint_every)
{
    if (B < 1 || S < 1 || N < 1 || H < 1 || W < 1 || horizon < 1 || checkpoint_every < 1) return 0;
    return sft_fit(workspace_needed(B, S, N, H, W, horizon, checkpoint_every));
}

int nastar_soft_routes_tiled(const float* cost, const float* goal, const float* passable, const void* tape, size_t tape_bytes,
                             int checkpoint_every, const int32_t* start_idx, int B, int S, int N, int H, int W, unsigned neighbor_mask,
                             double tau, int horizon, long long seed, const float* uniforms, int32_t* routes_out, int route_cap,
                             int32_t* route_len_out, float* route_cost_out, float* log_prob_out, int32_t* visits_out, int32_t* status_out,
                             void* workspace, size_t workspace_bytes, void* stream)
{
    const int c = checkpoint_every, K = horizon;
    if (!field_mask_ok(neighbor_mask)) return NASTAR_ERR_UNSUPPORTED;
    if (!cost || !goal || !passable || !tape || !start_idx || !route_len_out || !status_out || !workspace) return NASTAR_ERR_NULL;
    if (S < 1 || N < 1 || (routes_out && route_cap < 1)) return NASTAR_ERR_BAD_SHAPE;
    if (B < 1 || H < 1 || W < 1 || K < 1 || c < 1 || !(tau > 0.0) || !std::isfinite(tau)) return NASTAR_ERR_BAD_SHAPE;
    if (!tiled_shape_ok(B, H, W)) return NASTAR_ERR_UNSUPPORTED;  // above kTiledMaxCells cells, or more than 2^24 tiles in the batch
    if ((long long)S * N > kSoftRoutesTiledMaxWalkers || (long long)B * ((long long)S * N) > kSoftRoutesTiledMaxWalkers) return NASTAR_ERR_UNSUPPORTED;
    if (int rc = soft_tiled_call_ok(B, H, W, tau, K, c, 1, tape, tape_bytes, workspace, workspace_bytes,
                                    nastar_soft_routes_tiled_workspace_bytes(B, S, N, H, W, K, c)))
        return rc;  // (what is left of it: the tape and the workspace)

    const SoftTiledGeometry geo = soft_tiled_geometry(B, H, W);
    const int HW = H * W;
    const long long SN = (long long)S * N;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    int32_t* flags = reinterpret_cast<int32_t*>(ws);
    int32_t* map_status = reinterpret_cast<int32_t*>(ws + (size_t)sft_flag_bytes(B));  // (the prepare launch's; the forward has reported it)
    float* C = reinterpret_cast<float*>(ws + 2 * (size_t)sft_flag_bytes(B));
    const size_t stride = (size_t)sft_plane_bytes(B, H, W) / 4;
    float* V0 = C + stride;
    SoftRoutesTiledState* state = reinterpret_cast<SoftRoutesTiledState*>(C + 2 * stride);
    float* seg = reinterpret_cast<float*>(reinterpret_cast<char*>(state) + (size_t)state_bytes(B, S, N));
    const float* ck = static_cast<const float*>(tape);  // slot j - 1 is plane j * c; slot K / c is plane K

    if (int rc = soft_tiled_prepare(cost, goal, passable, C, V0, flags, map_status, B, HW, false, tau, s)) return rc;
    // every row starts as -1 (the walkers store cells only) and every visit count as 0 (they add)
    if (int rc = soft_routes_clear(routes_out, visits_out, B, S, SN, HW, route_cap, s)) return rc;

    // (the tape is kept in units of tau * ln 2 and a draw needs differences of it only: tau goes into the rebuilt sweeps' costs alone)
    SoftRoutesTiledArgs t{};
    t.a = SoftRoutesArgs{cost, goal, passable, nullptr, start_idx, uniforms, routes_out, route_len_out, route_cost_out, log_prob_out, visits_out,
                         status_out, (int)((SN + kSoftRoutesGatherT - 1) / kSoftRoutesGatherT), S, N, H, W, K, routes_out ? route_cap : 0,
                         neighbor_mask, (uint32_t)((unsigned long long)seed & 0xffffffffull), (uint32_t)((unsigned long long)seed >> 32)};
    t.plane_K = ck + (size_t)(K / c) * geo.plane;
    t.seg = seg;
    t.flags = flags;
    t.state = state;
    t.plane = geo.plane;
    const dim3 grid((unsigned)((long long)B * t.a.groups)), block(kSoftRoutesGatherT);

    // one pass over the segments, top down: every step is walked (lowest = 1), the first launch forms the walkers, the last is segment 0's
    auto pass = [&](auto first, int store) {
        t.store = store;
        t.begin = 1;
        return soft_tiled_each_segment(C, V0, ck, seg, K, c, 1, neighbor_mask, geo, s, [&](int lo, int hi, int, auto&& plane) {
            t.lo = lo;
            t.hi = hi;
            t.first = plane(lo);
            t.end = lo == 0;
            const int rc = launch_grid(nastar_soft_routes_tiled_kernel<decltype(first)::value>, grid, block, 0, s, t);
            t.begin = 0;
            return rc;
        });
    };
    if (!routes_out) return pass(std::true_type{}, kSrtStoreNone);
    if (route_cap >= K + 1) return pass(std::true_type{}, kSrtStoreRows);  // no route outgrows the row: store on the way
    // a walk that may outgrow its row is replayed, first for the lengths, then for the stores: every segment is rebuilt twice
    if (int rc = pass(std::true_type{}, kSrtStoreNone)) return rc;
    return pass(std::false_type{}, kSrtStoreTail);
}

}  // extern "C"
