// nastar_soft_routes_grad_capi.hip -- the C ABI of include/nastar_soft_routes_grad.h: the score-function backward of the sampled routes.  A
// translation unit of its own: nothing here touches the other field kernels; the field's backward is called through its own entry point.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "nastar_soft_fields_host.hip.h"
#include "nastar_soft_routes_grad.hip.h"

using namespace nastar;

constexpr long long kSoftRoutesGradMaxWalkers = 1ll << 30;
constexpr int kSoftRoutesGradMaxP = 40, kSoftRoutesGradMinP = 30;

static_assert(soft_routes_grad_lds_bytes(kSoftRoutesGradMaxCells) <= 64 * 1024, "the int64 plane of the largest map: 48 KiB, no raised LDS limit");
// No sum of the definition leaves int64: |q| <= 2^(P + 1) and a route has at most K cells but the last, so |Q_visit| <= S*N*K * 2^(P + 1)
// <= 2^ceil(log2(S*N*K)) * 2^(P + 1) <= 2^(61 - P) * 2^(P + 1) = 2^62 (P <= 61 - ceil(log2(S*N*K)) by its definition); Q_seed sums S*N of them.

// P of the definition for S*N*K = n >= 1 (n < 2^61: S*N <= 2^30 and K < 2^31)
static int soft_routes_grad_bits(long long n)
{
    const int ceil_log2 = n <= 1 ? 0 : 64 - __builtin_clzll((unsigned long long)(n - 1));
    return std::min(kSoftRoutesGradMaxP, 61 - ceil_log2);
}

// the workspace: Q_visit, Q_seed (int64), the seed plane, A32 (fp32), then the scale of every map
static size_t plane_bytes(int B, int H, int W) { return (size_t)B * (size_t)H * (size_t)W; }

extern "C" {

int nastar_soft_routes_grad_abi(void) { return NASTAR_SOFT_ROUTES_GRAD_ABI; }

int nastar_soft_routes_grad_max_cells(void) { return kSoftRoutesGradMaxCells; }

size_t nastar_soft_routes_grad_workspace_bytes(int B, int H, int W)
{
    if (B < 1 || H < 1 || W < 1) return 0;
    const unsigned __int128 n = (unsigned __int128)B * ((unsigned __int128)H * (unsigned)W) * 24u + (unsigned __int128)B * sizeof(SrgScale) + 15u;
    return n > (unsigned __int128)SIZE_MAX ? SIZE_MAX : (size_t)n / 16 * 16;
}

int nastar_soft_routes_backward(const float* cost, const float* goal, const float* passable, const void* tape, size_t tape_bytes,
                                const int32_t* start_idx, const int32_t* routes, int route_cap, const int32_t* route_len,
                                const int32_t* status, const float* grad_log_prob, int B, int S, int N, int H, int W, unsigned neighbor_mask,
                                double tau, int horizon, float* grad_cost_out, int32_t* status_out, void* workspace, size_t workspace_bytes,
                                void* stream)
{
    if (!field_mask_ok(neighbor_mask)) return NASTAR_ERR_UNSUPPORTED;
    if (!cost || !goal || !passable || !tape || !start_idx || !routes || !route_len || !status || !grad_log_prob || !grad_cost_out || !status_out)
        return NASTAR_ERR_NULL;
    if (B < 1 || S < 1 || N < 1 || H < 1 || W < 1 || horizon < 1 || !(tau > 0.0) || !std::isfinite(tau)) return NASTAR_ERR_BAD_SHAPE;
    if ((long long)route_cap < (long long)horizon + 1) return NASTAR_ERR_BAD_SHAPE;  // whole rows: no walk is replayed here
    if ((long long)H * W > kSoftRoutesGradMaxCells) return NASTAR_ERR_UNSUPPORTED;
    if ((long long)S * N > kSoftRoutesGradMaxWalkers || (long long)B * ((long long)S * N) > kSoftRoutesGradMaxWalkers) return NASTAR_ERR_UNSUPPORTED;
    const int P = soft_routes_grad_bits((long long)S * N * horizon);
    if (P < kSoftRoutesGradMinP) return NASTAR_ERR_UNSUPPORTED;
    if (int rc = soft_call_ok(B, H, W, tau, horizon, kSoftRoutesGradMaxCells, tape, tape_bytes)) return rc;  // (what is left of it: the tape)
    if (!workspace || workspace_bytes < nastar_soft_routes_grad_workspace_bytes(B, H, W) || !aligned16(workspace)) return NASTAR_ERR_WORKSPACE;

    const int HW = H * W;
    const size_t cells = plane_bytes(B, H, W);
    const long long SN = (long long)S * N;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    long long* q_visit = reinterpret_cast<long long*>(ws);
    long long* q_seed = q_visit + cells;
    float* seed = reinterpret_cast<float*>(q_seed + cells);
    float* a32 = seed + cells;
    SrgScale* scale = reinterpret_cast<SrgScale*>(a32 + cells);
    constexpr int T = kSoftRoutesGradT;
    SoftRoutesGradArgs a{start_idx, routes, route_len, status, grad_log_prob, q_visit, q_seed, scale,
                         (int)((SN + kSoftRoutesGradWalkers - 1) / kSoftRoutesGradWalkers), S, N, HW, horizon, route_cap, P};
    const dim3 flat((unsigned)std::min<size_t>((cells + T - 1) / T, 1u << 16));

    if (int rc = launch_grid(nastar_soft_routes_grad_scale_kernel<T>, dim3((unsigned)B), dim3(T), 0, s, a)) return rc;
    if (int rc = launch_grid(nastar_soft_routes_grad_histogram_kernel<T>, dim3((unsigned)((long long)B * a.groups)), dim3(T),
                             soft_routes_grad_lds_bytes(HW), s, a))
        return rc;
    if (int rc = launch_grid(nastar_soft_routes_grad_seed_kernel<T>, flat, dim3(T), 0, s, a, seed, cells)) return rc;
    // the field's backward on the seed plane, through its own entry point: the existing launch and its bits; it writes status_out
    if (int rc = nastar_soft_fields_backward(cost, goal, passable, tape, tape_bytes, seed, B, H, W, neighbor_mask, tau, horizon, a32, status_out, stream))
        return rc;
    return launch_grid(nastar_soft_routes_grad_combine_kernel<T>, flat, dim3(T), 0, s, a, (const float*)a32, (const int32_t*)status_out, tau,
                       grad_cost_out, cells);
}

}  // extern "C"
