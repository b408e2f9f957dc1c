// nastar_soft_fields.hip.h -- the entropy-regularised (soft-min) cost-to-go field of whole maps over a finite horizon, its soft policy, and
// its gradient with respect to the cost maps (include/nastar_soft_fields.h).
//
// One workgroup owns one map, as in nastar_fields.hip.h.  Both kernels work in UNITS of tau * ln 2: U = V / (tau * ln 2), so that the soft-min is
// min - log2(sum of exp2(min - x)) on the native v_exp_f32 / v_log_f32 with no multiply in front of either; the cost is scaled once at the
// load, the field once at the store, and the tape holds U.  The gradient needs neither factor: d V_K / d cost = d U_K / d (cost in units).
//
// FORWARD.  LDS holds three fp32 per cell:
//   C[i]    the cost in units with the obstacles folded in as +inf (fl32(+inf + x) is +inf: the sweep has no passable test) and the passable
//           goals as -1 (a cost is >= 0: the sweep writes 0 there);
//   V0, V1  two planes of the field, ping-ponged: sweep k reads plane k-1 ONLY and writes plane k (Jacobi), one barrier per sweep.  The result
//           is a pure function of the inputs, whatever order the wavefronts ran in.
// Exactly `horizon` sweeps: no trip count depends on the data.  With a tape every sweep also stores its plane (planes 1..horizon, coalesced).
//
// BACKWARD.  A_{k-1}(m) = sum over the predecessors n of m of pi_k(m|n) A_k(n), and pi_k(m|n) = exp2(M_k(n) - U_{k-1}(m)) / S_k(n) with M and S
// the minimum and the sum of sfl_softmin at n on plane k-1 -- kept APART, so that the exponent is a difference of two nearby fp32 values (a
// pi formed from U_k(n) - cost[n] - U_{k-1}(m) would carry the rounding of |U|, thousands of units at a small tau).  A step is two passes with
// a barrier behind each: every n writes P(n) = A_k(n) / S_k(n) and M_k(n); every m gathers, in the row-major order of kChildOffsets, adds the
// result to its fp64 sum and fetches its value of the next plane from the tape.  LDS per cell: the fp64 sum, A, P, M, the plane, and one byte
// that says "passable and no goal".  No floating-point atomics.
//
// Both kernels are thin wrappers of a body (sfl_forward, sfl_backward) with a compile-time switch: nastar_soft_policy.hip.h instantiates the
// other side of it, the log-policy and its adjoint.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/nastar_soft_fields.h"
#include "nastar_field_rules.hip.h"

namespace nastar {

constexpr int kSoftFieldsMaxCells = 12288;     // 3 x 4 B x 12288 = 144 KiB of the 160 KiB a workgroup may own
constexpr int kSoftFieldsGradMaxCells = 6144;  // 25 B x 6144 = 150 KiB

struct SoftFieldArgs {
    const float* cost;      // [B,HW]
    const float* goal;
    const float* passable;
    float* dist;            // [B,HW]
    float* policy;          // [B,8,HW] or nullptr
    int32_t* status;        // [B]
    float* tape;            // [B,horizon,HW] or nullptr
    int H, W, horizon;
    uint32_t nmask;
    float to_units;         // 1 / (tau ln 2)
    float from_units;       // tau ln 2
};

struct SoftFieldGradArgs {
    const float* cost;      // [B,HW]
    const float* goal;
    const float* passable;
    const float* tape;      // [B,horizon,HW]
    const float* grad_dist; // [B,HW] (sfl_backward<T, true>: or nullptr = zeros)
    float* grad_cost;       // [B,HW]
    int32_t* status;        // [B]
    int H, W, horizon;
    uint32_t nmask;
};

constexpr size_t sfl_pad16(size_t n) { return (n + 15) / 16 * 16; }
// LDS bytes of one map, forward: C, V0, V1, then the flags (has_goal [0], bad_cost [1])
constexpr size_t soft_fields_lds_bytes(int HW) { return sfl_pad16((size_t)HW * 12) + 32; }
// backward: the fp64 sums, A, P, M, the plane, the eligibility bytes, then the flags (bad_cost [1])
constexpr size_t soft_fields_grad_lds_bytes(int HW) { return (size_t)HW * 24 + sfl_pad16((size_t)HW) + 32; }

__device__ __forceinline__ float sfl_exp2(float x) { return __builtin_amdgcn_exp2f(x); }  // v_exp_f32: exp2(-inf) = 0
__device__ __forceinline__ float sfl_log2(float x) { return __builtin_amdgcn_logf(x); }   // v_log_f32, on [1, 8] here

// THE SOFT-MIN of one cell, in two parts: m = the smallest at(dy, dx) over the allowed in-map moves (+inf when there is none, or none with
// a finite target) and s = the sum of exp2(m - x) over them, in kChildOffsets order (0 when m is +inf, else 1 <= s <= 8).
struct SoftMin {
    float m, s;
};
template <typename At>
__device__ __forceinline__ SoftMin sfl_softmin(At at, uint32_t nm, bool up, bool dn, bool lf, bool rt)
{
    float x[8];
    float m = INFINITY;
    fld_each<8>([&](auto j) __attribute__((always_inline)) {
        constexpr Move o = kChildOffsets[decltype(j)::value];
        x[decltype(j)::value] = ((nm & fld_bit(o.dy, o.dx)) && fld_inside(o.dy, o.dx, up, dn, lf, rt)) ? at(o.dy, o.dx) : INFINITY;
        m = fminf(m, x[decltype(j)::value]);
    });
    const float base = m < INFINITY ? m : 0.f;  // (+inf - +inf is a NaN)
    float s = 0.f;
    fld_each<8>([&](auto j) __attribute__((always_inline)) { s += sfl_exp2(base - x[decltype(j)::value]); });
    return {m, s};
}

// the cells tid, tid + T, ... of a lane with their rows and columns, without a division per cell
template <int T, typename F>
__device__ __forceinline__ void sfl_cells(int HW, int W, F&& f)
{
    const int tid = threadIdx.x;
    int r = tid / W, c = tid - r * W;
    const int dr = T / W, dc = T - dr * W;
    for (int i = tid; i < HW; i += T) {
        f(i, r, c);
        r += dr;
        c += dc;
        if (c >= W) {
            c -= W;
            ++r;
        }
    }
}

// THE FORWARD of one map.  LOGP: the epilogue also writes the log-policy of include/nastar_soft_policy.h to log_policy [B,8,HW], from the M, S
// and plane K-1 the policy is formed from (nastar_soft_policy.hip.h); everything else is the same statements, so the same bits.
template <int T, bool LOGP>
__device__ __forceinline__ void sfl_forward(const SoftFieldArgs& a, float* log_policy)
{
    extern __shared__ __attribute__((aligned(16))) char sfl_smem[];
    const int H = a.H, W = a.W, HW = H * W, K = a.horizon;
    float* C = reinterpret_cast<float*>(sfl_smem);
    float* prev = C + HW;
    float* next = prev + HW;
    int* flags = reinterpret_cast<int*>(sfl_smem + sfl_pad16((size_t)HW * 12));
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * HW;
    const float* goal = a.goal + base;
    const float INF = INFINITY;

    if (tid < 8) flags[tid] = 0;
    __syncthreads();

    // ---- load -----------------------------------------------------------------------------------------------------------------------------
    bool has_goal = false, bad = false;
    for (int i = tid; i < HW; i += T) {
        const float c = a.cost[base + i], g = goal[i];
        const bool ok = a.passable[base + i] != 0.f;
        bad |= ok && !(c >= 0.f);  // NaN or negative on a passable cell (-0.0 >= 0)
        has_goal |= g != 0.f;
        C[i] = !ok ? INF : g != 0.f ? -1.f : c * a.to_units;
        prev[i] = (ok && g != 0.f) ? 0.f : INF;
    }
    if (__ballot(has_goal) && (tid & 63) == 0) __hip_atomic_store(&flags[0], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (__ballot(bad) && (tid & 63) == 0) __hip_atomic_store(&flags[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    const bool map_bad = flags[1] != 0, map_goal = flags[0] != 0;
    if (map_bad) {  // a map of +inf: the sweeps below run as for every other map, and the tape says "nothing is live"
        for (int i = tid; i < HW; i += T) {
            C[i] = INF;
            prev[i] = INF;
        }
    }
    __syncthreads();

    // ---- the sweeps ---------------------------------------------------------------------------------------------------------------------------
    const uint32_t nm = a.nmask;
    for (int k = 1; k <= K; ++k) {
        float* plane = a.tape ? a.tape + ((size_t)blockIdx.x * K + (k - 1)) * HW : nullptr;
        sfl_cells<T>(HW, W, [&](int i, int r, int c) {
            const float* at = prev + i;
            const SoftMin sm = sfl_softmin([&](int dy, int dx) { return at[dy * W + dx]; }, nm, r > 0, r < H - 1, c > 0, c < W - 1);
            const float cc = C[i];
            const float v = cc < 0.f ? 0.f : sm.m < INF ? cc + (sm.m - sfl_log2(sm.s)) : INF;
            next[i] = v;
            if (plane) plane[i] = v;
        });
        __syncthreads();
        float* t = prev;
        prev = next;
        next = t;
    }
    // prev is plane K, next plane K - 1

    // ---- epilogue: the field, then the policy planes, every store coalesced ---------------------------------------------------------------------
    if (tid == 0) a.status[blockIdx.x] = map_bad ? NASTAR_ERR_BAD_COST : !map_goal ? NASTAR_ERR_UNSOLVABLE : NASTAR_OK;
    float* dist = a.dist + base;
    for (int i = tid; i < HW; i += T) dist[i] = map_bad ? INF : goal[i] != 0.f ? 0.f : prev[i] * a.from_units;
    if (LOGP || a.policy) {
        float* pol = (!LOGP || a.policy) ? a.policy + base * 8 : nullptr;
        float* lpol = LOGP ? log_policy + base * 8 : nullptr;
        sfl_cells<T>(HW, W, [&](int i, int r, int c) {
            const bool up = r > 0, dn = r < H - 1, lf = c > 0, rt = c < W - 1;
            const float* at = next + i;
            const SoftMin sm = sfl_softmin([&](int dy, int dx) { return at[dy * W + dx]; }, nm, up, dn, lf, rt);
            const float cc = C[i];
            const bool live = cc >= 0.f && cc < INF && sm.m < INF;
            float log2s = 0.f;
            if constexpr (LOGP) log2s = sfl_log2(sm.s);
            fld_each<8>([&](auto k) __attribute__((always_inline)) {
                constexpr Move mv = kActionMoves[decltype(k)::value];
                float w = 0.f, lw = -INF;
                if (live && (nm & fld_bit(mv.dy, mv.dx)) && fld_inside(mv.dy, mv.dx, up, dn, lf, rt)) {
                    w = sfl_exp2(sm.m - at[mv.dy * W + mv.dx]) / sm.s;
                    // the minimum and the sum kept apart, as in w: -inf by itself for a target of +inf
                    if constexpr (LOGP) lw = ((sm.m - at[mv.dy * W + mv.dx]) - log2s) * (float)M_LN2;
                }
                if (!LOGP || pol) pol[(size_t) decltype(k)::value * HW + i] = w;
                if constexpr (LOGP) lpol[(size_t) decltype(k)::value * HW + i] = lw;
            });
        });
    }
}

template <int T>
__global__ __launch_bounds__(T) void nastar_soft_cost_to_go_kernel(const SoftFieldArgs a)
{
    sfl_forward<T, false>(a, nullptr);
}

// the second seed of the backward (include/nastar_soft_policy.h): the upstream gradient of the log-policy of ONE map, [8,HW], or nullptr
struct SoftPolicySeed {
    const float* grad_log_policy;
    float neg_inv_tau;  // -1 / tau
};

// THE BACKWARD of one map.  POLICY: a.grad_dist may be nullptr (zeros), and a log-policy seed GL is INJECTED AT STEP K (nastar_soft_policy.hip.h):
// A_{K-1} = the gather + Z.  Step K's first pass also leaves Q(n) = gsum(n) / S_K(n) and A_K(n) in the two halves of the cell's fp64 slot --
// the sum is A_K alone until that step's gather has run, so the slot is free -- the gather adds GL(a,n) - exp2(M(n) - u) Q(n) over the
// predecessors live at K, and a third pass makes the slot the sum again.  Without a seed every statement is the plain backward's: the same bits.
template <int T, bool POLICY>
__device__ __forceinline__ void sfl_backward(const SoftFieldGradArgs& a, const SoftPolicySeed seed)
{
    extern __shared__ __attribute__((aligned(16))) char sfg_smem[];
    const int H = a.H, W = a.W, HW = H * W, K = a.horizon;
    double* sum = reinterpret_cast<double*>(sfg_smem);
    float* A = reinterpret_cast<float*>(sfg_smem + (size_t)HW * 8);
    float* P = A + HW;
    float* M = P + HW;
    float* U = M + HW;
    uint8_t* elig = reinterpret_cast<uint8_t*>(sfg_smem + (size_t)HW * 24);
    int* flags = reinterpret_cast<int*>(sfg_smem + (size_t)HW * 24 + sfl_pad16((size_t)HW));
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * HW;
    const float* tape = a.tape + (size_t)blockIdx.x * K * HW;  // plane k is tape + (k - 1) * HW
    const float INF = INFINITY;

    if (tid < 8) flags[tid] = 0;
    __syncthreads();

    // ---- A_K: the upstream gradient on the cells live at K, 0 elsewhere (what is not live is never read) -----------------------------------------
    bool bad = false;
    for (int i = tid; i < HW; i += T) {
        const bool ok = a.passable[base + i] != 0.f;
        bad |= ok && !(a.cost[base + i] >= 0.f);
        const bool e = ok && a.goal[base + i] == 0.f;
        const bool live = e && tape[(size_t)(K - 1) * HW + i] < INF;
        float g = 0.f;
        if (live && (!POLICY || a.grad_dist)) g = a.grad_dist[base + i];
        elig[i] = POLICY ? e | (live ? 2 : 0) : e;  // (bit 1: live at K, what the injected step asks of a predecessor)
        A[i] = g;
        sum[i] = (double)g;
        U[i] = K >= 2 ? tape[(size_t)(K - 2) * HW + i] : INF;
    }
    if (__ballot(bad) && (tid & 63) == 0) __hip_atomic_store(&flags[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    const bool map_bad = flags[1] != 0;

    // ---- one step k: U holds plane k - 1; `inject` (a std::bool_constant) adds the log-policy seed, at step K only -----------------------------------
    const uint32_t nm = a.nmask;
    const float* gl = seed.grad_log_policy;
    float* slot = reinterpret_cast<float*>(sum);  // slot[2 i] = Q(i), slot[2 i + 1] = A_K(i) while the injected step runs
    auto step = [&](int k, auto inject) __attribute__((always_inline)) {
        constexpr bool kInject = decltype(inject)::value;
        sfl_cells<T>(HW, W, [&](int i, int r, int c) {
            const bool up = r > 0, dn = r < H - 1, lf = c > 0, rt = c < W - 1;
            const float* at = U + i;
            const SoftMin sm = sfl_softmin([&](int dy, int dx) { return at[dy * W + dx]; }, nm, up, dn, lf, rt);
            const bool any = sm.m < INF;  // (A is 0 on a cell that is not live at k, whatever its soft-min)
            P[i] = any ? A[i] / sm.s : 0.f;
            M[i] = any ? sm.m : -INF;     // exp2(-inf - u) = 0
            if constexpr (kInject) {
                float gsum = 0.f;
                if (elig[i] & 2) {  // live at K: GL is read on Act(i) only, in the row-major order of the move offsets
                    fld_each<8>([&](auto j) __attribute__((always_inline)) {
                        constexpr Move o = kChildOffsets[decltype(j)::value];
                        if ((nm & fld_bit(o.dy, o.dx)) && fld_inside(o.dy, o.dx, up, dn, lf, rt) && at[o.dy * W + o.dx] < INF)
                            gsum += gl[(size_t)kOppositeAction[7 - decltype(j)::value] * HW + i];
                    });
                }
                slot[2 * i] = gsum / sm.s;  // (S >= 1 on a live cell; what is not live is 0 / S or 0 / 0 and is never read)
                slot[2 * i + 1] = A[i];
            }
        });
        __syncthreads();
        const float* below = k > 2 ? tape + (size_t)(k - 3) * HW : nullptr;  // plane k - 2
        sfl_cells<T>(HW, W, [&](int i, int r, int c) {
            const bool up = r > 0, dn = r < H - 1, lf = c > 0, rt = c < W - 1;
            const float u = U[i];
            float acc = 0.f, z = 0.f;
            // the predecessor at kChildOffsets[j] steps onto this cell by the opposite move
            fld_each<8>([&](auto j) __attribute__((always_inline)) {
                constexpr Move o = kChildOffsets[decltype(j)::value];
                if ((nm & fld_bit(-o.dy, -o.dx)) && fld_inside(o.dy, o.dx, up, dn, lf, rt)) {
                    const int n = i + o.dy * W + o.dx;
                    const float w = sfl_exp2(M[n] - u);
                    acc += P[n] * w;
                    if constexpr (kInject) {
                        if ((elig[n] & 2) && u < INF) z += gl[(size_t)kOppositeAction[decltype(j)::value] * HW + n] - w * slot[2 * n];
                    }
                }
            });
            float v = acc;
            if constexpr (kInject) v = acc + z * seed.neg_inv_tau;
            v = (elig[i] && u < INF) ? v : 0.f;
            A[i] = v;
            if constexpr (!kInject) sum[i] += (double)v;
            if (below) U[i] = below[i];
        });
        __syncthreads();
        if constexpr (kInject) {  // the slot is the sum again: A_K + A_{K-1}, the two additions the plain step makes
            for (int i = tid; i < HW; i += T) {
                const float g = slot[2 * i + 1];
                sum[i] = (double)g + (double)A[i];
            }
        }
    };

    // ---- steps k = K .. 2 -------------------------------------------------------------------------------------------------------------------------
    int k = K;
    if constexpr (POLICY) {
        if (gl && k >= 2) step(k--, std::true_type{});
    }
    for (; k >= 2; --k) step(k, std::false_type{});

    // ---- epilogue: one rounding per cell -----------------------------------------------------------------------------------------------------
    if (tid == 0) a.status[blockIdx.x] = map_bad ? NASTAR_ERR_BAD_COST : NASTAR_OK;
    for (int i = tid; i < HW; i += T) a.grad_cost[base + i] = map_bad ? 0.f : (float)sum[i];
}

template <int T>
__global__ __launch_bounds__(T) void nastar_soft_fields_backward_kernel(const SoftFieldGradArgs a)
{
    sfl_backward<T, false>(a, SoftPolicySeed{nullptr, 0.f});
}

}  // namespace nastar
