// nastar_backward_replay.hip.h -- backward of DifferentiableAstar.forward (differentiable_astar.py:203-252 under autograd),
// round-2 algorithm: REPLAY the search from the forward's selection log and account the softmax gradient per EVENT.
//
//     dL/dcost = sum_t kfac * y_t * (G - <G, y_t>),   y_t = v / S_t over the open list,  v_i = exp(-q_i),  kfac = (1-g_ratio)(-1/sqrt(W))
//
// The round-1 kernels re-evaluated the whole softmax (two wave sums, one exp per open cell) before EVERY selection: O(open list)
// per step, 3.7x the cost of a forward step.  Between two re-keyings a cell's v_i is constant, so its gradient over an interval
// [t0, t1] of steps on the open list is   kfac * v_i * (G_i * (A(t1) - A(t0)) - (B(t1) - B(t0)))   with the running sums
//     A(t) = sum_{tau <= t} w_tau / S_tau,      B(t) = sum_{tau <= t} w_tau * D_tau / S_tau^2,      D_t = sum_open v * G
// and S, D change by at most 9 cells per step (the closed node and its <= 8 relaxed neighbours): O(9) per step.
//   * S, D live in LDS as doubles and are updated with ds_add_f64 by the <= 9 lanes that change them; a cell's v enters and
//     leaves with the identical fp32 value, and fp64 adds fp32 terms exactly, so S and D carry no drift (the reference sums in fp32).
//   * A, B are doubles in registers (wave-uniform).  Every step appends (A, B) to a per-map history in the HBM workspace; a cell
//     stores the step that opened it (u16 in LDS) and its interval is closed with one 16-byte history load, consumed one step later
//     (software-pipelined: never on the replay's critical path).
//   * contributions go to grad_cost with global_atomic_add_f32 (fire and forget); cells still open at the end are flushed by a sweep.
//   * no selection at all: s_t comes from the forward's sel_log, so a step is one LDS round trip.
// w_tau = 1 except for the reference's batch-coupled fixed-point steps (`extra`, see nastar_backward in include/nastar.h).
// Prototype with the same arithmetic, checked against the reference's autograd: tools/proto_backward_events.py.
#pragma once
#include <type_traits>

#include "nastar_search_compact.hip.h"

namespace nastar {

struct BwdRArgs {
    const float* grad_hist;  // upstream dL/dhistories, or nullptr: L1 loss fused (l1_* below)
    const float* l1_hist;
    const float* l1_traj;
    const float* l1_up;
    float l1_scale;
    const float* cost;
    const float* start;
    const float* goal;
    const float* passable;
    const int* sel_log;   // [B, max_iters] selections of the forward
    const int* iters;     // [B]
    const int* t_batch;   // device scalar or nullptr
    const int* order;     // optional placement (workgroup i replays map order[i]); nullptr = identity
    const int* order_bad; // optional verdict of nastar_order_check_kernel (NASTAR_FLAG_CHECK_ORDER): != 0 = ignore `order`
    int B_total;          // maps in the batch (bounds the placement)
    float* grad_cost;     // [B,H,W], fully written by this kernel
    double* hist;         // workspace: [B][hist_len][2]  (A, B) after each step; entry 0 = (0, 0)
    unsigned char* state; // workspace for maps whose state does not fit LDS (kGlobal), else nullptr
    size_t state_stride;
    int max_iters;
    int hist_len;  // history entries per map = min(max_iters, HW + 1) + 2
    float kfac;
    CompactDims d;
};

// gc 8 + G 4 + t0 2 per cell (wide: t0 4 -- history stamps beyond 65535: the HBM state of maps above 65,519 cells), + (S, D)
__host__ __device__ inline size_t bwdr_state_bytes(int HWp, bool wide = false) { return (size_t)HWp * (wide ? 16 : 14) + 64; }

__device__ __forceinline__ float bwdr_upstream(const BwdRArgs& a, size_t i)
{
    if (a.grad_hist != nullptr) return a.grad_hist[i];
    const float dlt = a.l1_hist[i] - a.l1_traj[i];  // fused L1 (training.py:58): sign(histories - opt_trajs) * grad / numel
    const float sg = dlt > 0.f ? 1.f : (dlt < 0.f ? -1.f : 0.f);
    return sg * (a.l1_scale * (a.l1_up != nullptr ? *a.l1_up : 1.f));
}

// state accessors: LDS, or the HBM workspace through the CU's vector L1.  The slab and the history of a map are touched by ONE wavefront
// between the fill and the sweep launch, and the lanes of a wavefront are coherent through their L1 without further action (write-through,
// accesses processed in order; global_step_fence per step) -- the neighbourhood of s* is mostly that of the previous step, i.e. L1 hits.
// (Rounds 2-5 used agent-scope relaxed atomics = sc1, served by L2: the forward's large-map kernel made the same move in round 5, 1275 -> 986 ns.)
template <bool kGlobal, typename T>
__device__ __forceinline__ T st_ld(const T* p)
{
    return *p;
}
template <bool kGlobal, typename T>
__device__ __forceinline__ void st_st(T* p, T v)
{
    *p = v;
}

template <bool kLds>
__device__ __forceinline__ double hist_ld(const double* p)
{
    return *p;
}
template <bool kLds>
__device__ __forceinline__ void hist_st(double* p, double v)
{
    *p = v;
}

// q = fl(f / fl32(sqrt(W))) of a cell with g-value G and hh = (1-g_ratio)(h0 + cost)   (:206-207); exp(-q) by v_exp_f32
template <bool kFastDiv>
__device__ __forceinline__ float bwdr_v(const CompactDims& d, float G, float hh, float rcp_sqrtW)
{
    const float f = d.gr * G + hh;
    float q;
    if constexpr (kFastDiv) {  // correctly rounded f / sqrt(W) for the verified widths (tools/fastdiv_check.c)
        const float q0 = f * rcp_sqrtW;
        const float rem = __builtin_fmaf(-q0, d.sqrtW, f);
        q = __builtin_fmaf(rem, rcp_sqrtW, q0);
    } else {
        q = f / d.sqrtW;
    }
    return __builtin_amdgcn_exp2f(q * -1.4426950408889634f);
}

// ---- maps whose state lives in the HBM workspace (kGlobal): the per-cell passes are launches of their own --------------------------------
// One wavefront initialising and, at the end, sweeping 262144 cells took ~10 ms per 512x512 map (its loop body is five agent-scope stores);
// as in the forward (nastar_search_hybrid.hip.h: fill / search / store) the two O(cells) passes run on ALL CUs and the one-wavefront-per-map
// launch between them does the O(steps) replay only.  Slab of a map: g | cost | G | t0 (bwdr_state_bytes) and, in its last 64 bytes, a header
// {int start, int goal, double A, double B}: start / goal cells found by the fill launch (atomicMax on -1), the final running sums left by
// the replay for the sweep.
__host__ __device__ inline size_t bwdr_header_offset(int HWp, bool wide) { return bwdr_state_bytes(HWp, wide) - 64; }

template <bool kWide>
__global__ __launch_bounds__(256) void nastar_bwdr_fill_kernel(const BwdRArgs a)
{
    using stamp_t = typename std::conditional<kWide, uint32_t, unsigned short>::type;
    const int b = blockIdx.y;
    const CompactDims& d = a.d;
    unsigned char* base = a.state + (size_t)b * a.state_stride;
    float* g = reinterpret_cast<float*>(base);
    float* cst = g + d.HWp;
    float* G = cst + d.HWp;
    stamp_t* t0 = reinterpret_cast<stamp_t*>(G + d.HWp);
    int* hdr = reinterpret_cast<int*>(base + bwdr_header_offset(d.HWp, kWide));  // {-1, -1, ..} on entry (nastar_hybrid_header_kernel)
    const size_t off = (size_t)b * (size_t)d.HW;
    float* gout = a.grad_cost + off;
    int sidx = -1, gidx = -1;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < d.HW; i += gridDim.x * 256) {
        if (a.start[off + i] != 0.f) sidx = i;
        if (a.goal[off + i] != 0.f) gidx = i;
        g[i] = a.passable[off + i] != 0.f ? NASTAR_POS_INF : NASTAR_NEG_INF;
        cst[i] = a.cost[off + i];
        G[i] = bwdr_upstream(a, off + i);
        t0[i] = (stamp_t)0;
        gout[i] = 0.f;
    }
    if (sidx >= 0) atomicMax(&hdr[0], sidx);
    if (gidx >= 0) atomicMax(&hdr[1], gidx);
}

// cells still on the open list when the replay ended: their intervals close at the final (A, B) the replay left in the header
// kHeur (nastar_bwdr_sweep_heuristic_kernel below): h0 is read from the caller's heuristic maps `h0p`
template <bool kWide, bool kFastDiv, bool kHeur>
__device__ __forceinline__ void bwdr_sweep(const BwdRArgs& a, const float rcp_sqrtW, const float* __restrict__ h0p)
{
    using stamp_t = typename std::conditional<kWide, uint32_t, unsigned short>::type;
    const int b = blockIdx.y;
    const CompactDims& d = a.d;
    const unsigned char* base = a.state + (size_t)b * a.state_stride;
    const float* g = reinterpret_cast<const float*>(base);
    const float* cst = g + d.HWp;
    const float* G = cst + d.HWp;
    const stamp_t* t0 = reinterpret_cast<const stamp_t*>(G + d.HWp);
    const int* hdr = reinterpret_cast<const int*>(base + bwdr_header_offset(d.HWp, kWide));
    const int sidx = hdr[0], gidx = hdr[1];
    if (sidx < 0 || gidx < 0) return;  // not a one-hot start / goal map: no replay ran, the gradient stays zero
    const double A = *reinterpret_cast<const double*>(hdr + 2), B = *reinterpret_cast<const double*>(hdr + 4);
    const double* hist = a.hist + (size_t)b * (size_t)a.hist_len * 2;
    float* gout = a.grad_cost + (size_t)b * (size_t)d.HW;
    const int goal_r = gidx / d.W, goal_c = gidx - goal_r * d.W;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < d.HW; i += gridDim.x * 256) {
        const float gi = g[i];
        if (fabsf(gi) < NASTAR_POS_INF) {
            const int ti = (int)t0[i];
            const double A0 = hist[2 * ti], B0 = hist[2 * ti + 1];
            const int ri = i / d.W, ci = i - ri * d.W;
            float h0v;
            if constexpr (kHeur) h0v = h0p[(size_t)b * (size_t)d.HW + i];
            else h0v = kWide ? heuristic0(ri, ci, goal_r, goal_c) : heuristic0_fast(ri, ci, goal_r, goal_c);
            const float v = bwdr_v<kFastDiv>(d, gi, d.omg * (h0v + cst[i]), rcp_sqrtW);
            const float dA = (float)(A - A0), dB = (float)(B - B0);
            gout[i] += (a.kfac * v) * (G[i] * dA - dB);  // (the replay's atomics are over: one thread per cell)
        }
    }
}

template <bool kWide, bool kFastDiv>
__global__ __launch_bounds__(256) void nastar_bwdr_sweep_kernel(const BwdRArgs a, const float rcp_sqrtW)
{
    bwdr_sweep<kWide, kFastDiv, false>(a, rcp_sqrtW, nullptr);
}

template <bool kWide, bool kFastDiv>
__global__ __launch_bounds__(256) void nastar_bwdr_sweep_heuristic_kernel(const BwdRArgs a, const float rcp_sqrtW, const float* __restrict__ h0p)
{
    bwdr_sweep<kWide, kFastDiv, true>(a, rcp_sqrtW, h0p);
}

// kHistLds: the (A, B) history lives in LDS behind the state (16 B per executed step): no global round trip inside the loop
// (an HBM history costs a write-through store + a vmcnt(0) drain per step, ~1 us).  kFastDiv: see compact_key.
// kWide (with kGlobal): maps above 65,519 cells / histories beyond 65535 entries -- 32-bit history stamps, and the heuristic with the
// correctly rounded square root (coordinates differences reach past 140: nastar_device.hip.h, sqrt_rn_int)
// kMasked (nastar_backward_replay_masked_kernel): the open sets are rebuilt with the neighbourhood of DifferentiableAstar.neighbor_filter
// (nmask, see neighbour_enabled), as the forward that wrote the log searched them.  Both kernels share one body, nastar_backward_replay_body.inc.
template <bool kGlobal, bool kHistLds, bool kFastDiv, bool kWide = false>
__global__ __launch_bounds__(64) void nastar_backward_replay_kernel(const BwdRArgs a, const float rcp_sqrtW)
{
    constexpr bool kMasked = false, kHeur = false, kMulti = false;
    constexpr uint32_t nmask = 0x1EFu;  // (NASTAR_NEIGHBORS_MOORE8; never read)
    constexpr const float* h0p = nullptr;
#include "nastar_backward_replay_body.inc"
}

template <bool kGlobal, bool kHistLds, bool kFastDiv, bool kWide = false>
__global__ __launch_bounds__(64) void nastar_backward_replay_masked_kernel(const BwdRArgs a, const float rcp_sqrtW, const uint32_t nmask)
{
    constexpr bool kMasked = true, kHeur = false, kMulti = false;
    constexpr const float* h0p = nullptr;
#include "nastar_backward_replay_body.inc"
}

// the replay of a search that ran with a caller-supplied heuristic (nastar_backward_replay_ordered_heuristic): the keys are rebuilt from
// `h0p`, the tensor the forward searched with; it always takes the neighbourhood mask.  dL/dh0 is the tensor this kernel writes for the
// cost (the loss sees both only through h = h0 + cost: g is detached every step, differentiable_astar.py:239).
template <bool kGlobal, bool kHistLds, bool kFastDiv, bool kWide = false>
__global__ __launch_bounds__(64) void nastar_backward_replay_heuristic_kernel(const BwdRArgs a, const float rcp_sqrtW, const uint32_t nmask,
                                                                              const float* __restrict__ h0p)
{
    constexpr bool kMasked = true, kHeur = true, kMulti = false;
#include "nastar_backward_replay_body.inc"
}

// the replay of a MULTI-SOURCE search (include/nastar_sources.h: nastar_backward_replay_sources): every non-zero cell of the start map is open
// from history index 0.  kHeur = false: the masked kernel's replay (h0p is not read); kHeur = true: the heuristic kernel's.
template <bool kGlobal, bool kHistLds, bool kFastDiv, bool kHeur, bool kWide = false>
__global__ __launch_bounds__(64) void nastar_backward_replay_sources_kernel(const BwdRArgs a, const float rcp_sqrtW, const uint32_t nmask,
                                                                            const float* __restrict__ h0p)
{
    constexpr bool kMasked = true, kMulti = true;
#include "nastar_backward_replay_body.inc"
}

}  // namespace nastar
