// nastar_soft_routes_capi.hip -- the C ABI of include/nastar_soft_routes.h: sampled routes from the maximum-entropy route distribution of the
// soft field.  A translation unit of its own: nothing here touches the other field kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "nastar_soft_fields_host.hip.h"
#include "nastar_soft_routes.hip.h"

using namespace nastar;

constexpr long long kSoftRoutesMaxWalkers = 1ll << 30;
// THE DISPATCH between the two kernel shapes, by measurement: up to this many walkers per map the tape is
// streamed through LDS -- 5-19 % ahead of the gathers at 16, 64 and 256 walkers on 32x32, 64x64 and 96x128 maps; above it every lane
// gathers -- 1.5-1.6 x ahead at 1024 and 4096.  A move is VALU issue (Philox, the draw, an fp64 log), so what counts is how many CUs the
// walkers are spread over: the streaming workgroup is as wide as the map needs (1024 lanes above 1024 cells), the gathering one 256.
constexpr long long kSoftRoutesLdsWalkers = 256;

static_assert(soft_routes_lds_bytes(kSoftRoutesMaxCells, true) <= kMaxLdsBytes, "two planes and the goal bytes of the largest map fit one workgroup's LDS");
static_assert(kSoftRoutesMaxCells <= 12 * 1024 && 1024 <= 4 * 256 && 256 <= 4 * 64, "a lane stages R cells of a plane: R * T covers every map its width T takes");

enum { kShapeAuto = 0, kShapeLds = 1, kShapeGather = 2 };

namespace nastar {

int soft_routes_clear(int32_t* routes, int32_t* visits, int B, int S, long long SN, int HW, int cap, hipStream_t s)
{
    if (!routes && !visits) return NASTAR_OK;
    const size_t n_routes = routes ? (size_t)B * SN * (size_t)cap : 0, n_visits = visits ? (size_t)B * S * (size_t)HW : 0;
    const size_t blocks = (std::max(n_routes, n_visits) + kSoftRoutesClearT - 1) / kSoftRoutesClearT;
    return launch_grid(nastar_soft_routes_clear_kernel<kSoftRoutesClearT>, dim3((unsigned)std::min<size_t>(blocks, 1u << 16)), dim3(kSoftRoutesClearT),
                       0, s, routes, n_routes, visits, n_visits);
}

}  // namespace nastar

static int soft_routes(const float* cost, const float* goal, const float* passable, const void* tape, size_t tape_bytes, const int32_t* start_idx,
                       int B, int S, int N, int H, int W, unsigned neighbor_mask, double tau, int horizon, long long seed, const float* uniforms,
                       int32_t* routes_out, int route_cap, int32_t* route_len_out, float* route_cost_out, float* log_prob_out,
                       int32_t* visits_out, int32_t* status_out, int shape, void* stream)
{
    if (!field_mask_ok(neighbor_mask)) return NASTAR_ERR_UNSUPPORTED;
    if (!cost || !goal || !passable || !tape || !start_idx || !route_len_out || !status_out) return NASTAR_ERR_NULL;
    if (S < 1 || N < 1 || (routes_out && route_cap < 1) || shape < kShapeAuto || shape > kShapeGather) return NASTAR_ERR_BAD_SHAPE;
    if (B < 1 || H < 1 || W < 1 || horizon < 1 || !(tau > 0.0) || !std::isfinite(tau)) return NASTAR_ERR_BAD_SHAPE;
    if ((long long)H * W > kSoftRoutesMaxCells || (long long)S * N > kSoftRoutesMaxWalkers || (long long)B * ((long long)S * N) > kSoftRoutesMaxWalkers)
        return NASTAR_ERR_UNSUPPORTED;
    if (int rc = soft_call_ok(B, H, W, tau, horizon, kSoftRoutesMaxCells, tape, tape_bytes)) return rc;  // (what is left of it: the tape)
    const int HW = H * W;
    const long long SN = (long long)S * N;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // (the tape is kept in units of tau * ln 2 and a draw needs differences of it only: tau is checked and not used)
    SoftRoutesArgs a{cost, goal, passable, static_cast<const float*>(tape), start_idx, uniforms, routes_out, route_len_out, route_cost_out,
                     log_prob_out, visits_out, status_out, 0, S, N, H, W, horizon, routes_out ? route_cap : 0, neighbor_mask,
                     (uint32_t)((unsigned long long)seed & 0xffffffffull), (uint32_t)((unsigned long long)seed >> 32)};
    // every row starts as -1 (the walkers store cells only) and every visit count as 0 (they add): one launch in front of the walkers'
    if (int rc = soft_routes_clear(routes_out, visits_out, B, S, SN, HW, route_cap, s)) return rc;
    const bool lds = shape == kShapeAuto ? SN <= kSoftRoutesLdsWalkers : shape == kShapeLds;
    auto go = [&](auto kernel, int T) {
        a.groups = (int)((SN + T - 1) / T);
        return launch_grid(kernel, dim3((unsigned)((long long)B * a.groups)), dim3(T), soft_routes_lds_bytes(HW, lds), s, a);
    };
    if (!lds) return go(nastar_soft_routes_kernel<kSoftRoutesGatherT, 1, false>, kSoftRoutesGatherT);
    // the widths of the forward (with_soft_block): what loads a plane per move is wavefronts
    return with_soft_block(HW, [&](auto T) { return go(nastar_soft_routes_kernel<T(), (T() == 1024 ? 12 : 4), true>, T()); });
}

extern "C" {

int nastar_soft_routes_abi(void) { return NASTAR_SOFT_ROUTES_ABI; }

int nastar_soft_routes_max_cells(void) { return kSoftRoutesMaxCells; }

int nastar_soft_routes(const float* cost, const float* goal, const float* passable, const void* tape, size_t tape_bytes,
                       const int32_t* start_idx, int B, int S, int N, int H, int W, unsigned neighbor_mask, double tau, int horizon,
                       long long seed, const float* uniforms, int32_t* routes_out, int route_cap, int32_t* route_len_out,
                       float* route_cost_out, float* log_prob_out, int32_t* visits_out, int32_t* status_out, void* stream)
{
    return soft_routes(cost, goal, passable, tape, tape_bytes, start_idx, B, S, N, H, W, neighbor_mask, tau, horizon, seed, uniforms, routes_out,
                       route_cap, route_len_out, route_cost_out, log_prob_out, visits_out, status_out, kShapeAuto, stream);
}

int nastar_soft_routes_with_shape(const float* cost, const float* goal, const float* passable, const void* tape, size_t tape_bytes,
                                  const int32_t* start_idx, int B, int S, int N, int H, int W, unsigned neighbor_mask, double tau,
                                  int horizon, long long seed, const float* uniforms, int32_t* routes_out, int route_cap,
                                  int32_t* route_len_out, float* route_cost_out, float* log_prob_out, int32_t* visits_out,
                                  int32_t* status_out, int shape, void* stream)
{
    return soft_routes(cost, goal, passable, tape, tape_bytes, start_idx, B, S, N, H, W, neighbor_mask, tau, horizon, seed, uniforms, routes_out,
                       route_cap, route_len_out, route_cost_out, log_prob_out, visits_out, status_out, shape, stream);
}

}  // extern "C"
