// nastar_soft_fields_tiled.hip.h -- the entropy-regularised cost-to-go field, its soft policy and its gradient for maps above the LDS of one
// workgroup (include/nastar_soft_fields_tiled.h).
//
// The definition and every expression of a cell's update are those of nastar_soft_fields.hip.h: sfl_softmin, `cc + (m - log2(s))`, `A / s`
// and `exp2(M - u)` in units of tau * ln 2 -- the results are the same bits.  What differs: the planes live in device memory as [B,HW] fp32
// in units, and a workgroup owns a TILE of a plane instead of a map.
//
// PREPARE (one workgroup per map): the bad-cost and has-goal flags, the status, and two planes: C, the cost in units with the obstacles
// folded in as +inf and the passable goals as -1 (C of the one-workgroup kernel, all +inf on a bad map), and V_0.
//
// SWEEPS (one workgroup per tile, n <= kSoftTileSweeps sweeps per launch): the workgroup loads C and plane k0 on its tile and a halo of n
// cells (+inf outside the map), and runs n Jacobi sweeps in LDS on a region that shrinks by one ring per sweep: after sweep s the cells at
// least s rings inside the loaded region hold plane k0 + s exactly -- the tile's interior after all n.  A sweep stores its interior where a
// plane is wanted: the launch's last into dst, a checkpoint into its slot of the tape.  The launch that reaches plane K holds plane K - 1
// on the interior and one ring, and writes dist and the policy as the one-workgroup epilogue does.  Nothing is read that another
// workgroup of the same launch writes.
//
// STEP of the backward (one workgroup per tile, one launch per k): plane k - 1 on the tile and two rings and A_k on one ring; every cell n
// of the tile and one ring writes P(n) = A_k(n) / S_k(n) and M_k(n); every cell m of the interior gathers in kChildOffsets order, stores
// A_{k-1}(m) into the other A plane and adds it to its fp64 sum in device memory.  One workgroup owns a cell: no atomics.
//
// The sweeps, init and step kernels carry a compile-time switch, off by default: nastar_soft_policy_tiled.hip.h instantiates the other side
// of it, the log-policy and its adjoint (item 6o).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nastar_soft_fields_tiled.h"
#include "nastar_soft_fields.hip.h"
#include "nastar_tile_geometry.hip.h"

namespace nastar {

constexpr int kSoftTileSweeps = 8;   // S: the sweeps of a launch and the rings of its halo (measured: DESIGN.md item 6m)
constexpr int kSoftTileT = 1024;     // lanes of a workgroup of the sweep and step kernels
constexpr int kSoftPlaneT = 256;     // ... of the cell-wise kernels

// LDS of a sweep launch of n sweeps: C and two planes on (kTileH + 2n) x (kTileW + 2n) cells
constexpr size_t soft_tile_lds_bytes(int n) { return (size_t)(kTileH + 2 * n) * (kTileW + 2 * n) * 12; }
// ... of a step launch: plane k - 1 on two rings, A (then P) and M on one
constexpr size_t soft_tile_grad_lds_bytes() { return ((size_t)(kTileH + 4) * (kTileW + 4) + 2 * (size_t)(kTileH + 2) * (kTileW + 2)) * 4; }
// ... of the step that injects the log-policy seed: Q beside P and M, and a byte "live at K" per cell of the one ring
constexpr size_t soft_tile_inject_lds_bytes() { return soft_tile_grad_lds_bytes() + (size_t)(kTileH + 2) * (kTileW + 2) * 5; }

struct SoftPrepareArgs {
    const float* cost;      // [B,HW]
    const float* goal;
    const float* passable;
    float* C;               // [B,HW]
    float* V0;              // [B,HW]
    int32_t* flags;         // [B,2]: has_goal, bad_cost
    int32_t* status;        // [B]
    int HW;
    int report_no_goal;     // the forward's status says NASTAR_ERR_UNSOLVABLE, the backward's does not
    float to_units;         // 1 / (tau ln 2)
};

struct SoftTileArgs {
    const float* C;         // [B,HW]
    const float* src;       // plane k0
    float* dst;             // plane k0 + n, or nullptr
    float* tape;            // slots of [B,HW], or nullptr
    const float* goal;      // (the launch that reaches K)
    const int32_t* flags;
    float* dist;
    float* policy;          // [B,8,HW] or nullptr
    TileGrid g;
    int k0, n;
    int tape_k0, tape_every, tape_count;  // plane k goes to slot (k - tape_k0) / tape_every - 1 when that is a whole number in 0 .. tape_count - 1
    int final_k, final_slot;              // ... and plane final_k to final_slot (-1: none)
    int last;                             // k0 + n is the horizon: write dist and the policy
    uint32_t nmask;
    float from_units;       // tau ln 2
};

struct SoftTileGradArgs {
    const float* C;         // [B,HW]
    const float* U;         // plane k - 1 (the step), plane K (the first launch)
    const float* A_in;      // A_k
    float* A_out;           // A_{k-1}
    double* sum;            // [B,HW]
    const float* grad_dist;
    float* grad_cost;
    const int32_t* flags;
    TileGrid g;
    uint32_t nmask;
};

template <int T>
__global__ __launch_bounds__(T) void nastar_soft_tiled_prepare_kernel(const SoftPrepareArgs a)
{
    __shared__ int flags[2];
    const int tid = threadIdx.x, HW = a.HW;
    const size_t base = (size_t)blockIdx.x * HW;
    const float INF = INFINITY;
    if (tid < 2) flags[tid] = 0;
    __syncthreads();
    bool has_goal = false, bad = false;
    for (int i = tid; i < HW; i += T) {
        const bool ok = a.passable[base + i] != 0.f;
        bad |= ok && !(a.cost[base + i] >= 0.f);  // NaN or negative on a passable cell (-0.0 >= 0)
        has_goal |= a.goal[base + i] != 0.f;
    }
    if (__ballot(has_goal) && (tid & 63) == 0) __hip_atomic_store(&flags[0], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (__ballot(bad) && (tid & 63) == 0) __hip_atomic_store(&flags[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    const bool map_bad = flags[1] != 0, map_goal = flags[0] != 0;
    for (int i = tid; i < HW; i += T) {
        const float c = a.cost[base + i], g = a.goal[base + i];
        const bool ok = a.passable[base + i] != 0.f;
        a.C[base + i] = (map_bad || !ok) ? INF : g != 0.f ? -1.f : c * a.to_units;
        a.V0[base + i] = (!map_bad && ok && g != 0.f) ? 0.f : INF;
    }
    if (tid == 0) {
        a.flags[2 * blockIdx.x] = map_goal;
        a.flags[2 * blockIdx.x + 1] = map_bad;
        a.status[blockIdx.x] = map_bad ? NASTAR_ERR_BAD_COST : (!map_goal && a.report_no_goal) ? NASTAR_ERR_UNSOLVABLE : NASTAR_OK;
    }
}

// the cells tid, tid + T, ... of a rows x cols block as f(row, column), without a division per cell
template <int T, typename F>
__device__ __forceinline__ void sft_cells(int rows, int cols, F&& f)
{
    const int tid = threadIdx.x, cnt = rows * cols;
    int r = tid / cols, c = tid - r * cols;
    const int dr = T / cols, dc = T - dr * cols;
    for (int i = tid; i < cnt; i += T) {
        f(r, c);
        r += dr;
        c += dc;
        if (c >= cols) {
            c -= cols;
            ++r;
        }
    }
}

// THE SWEEPS of one tile.  LOGP: the epilogue of the launch that reaches plane K also writes the log-policy of include/nastar_soft_policy.h to
// log_policy [B,8,HW], from the M, S and plane K-1 the policy is formed from (nastar_soft_policy_tiled.hip.h); everything else is the same
// statements, so the same bits.  The switch sits on the KERNEL, not on a body behind a wrapper: the plain instantiation then keeps its
// instruction stream too (tools/compare_device_code.py; log_policy is nullptr there and never looked at).
template <int T, bool LOGP = false>
__global__ __launch_bounds__(T) void nastar_soft_tiled_sweeps_kernel(const SoftTileArgs a, float* log_policy)
{
    extern __shared__ __attribute__((aligned(16))) char sft_smem[];
    const TilePos p = tld_pos(a.g);
    const int H = a.g.H, W = a.g.W, n = a.n;
    const int RH = p.rows + 2 * n, RW = p.cols + 2 * n, RN = RH * RW;  // the loaded region; its cell (0, 0) is the map's (y0 - n, x0 - n)
    const int ry = p.y0 - n, rx = p.x0 - n;
    float* C = reinterpret_cast<float*>(sft_smem);
    float* prev = C + RN;
    float* next = prev + RN;
    const float INF = INFINITY;
    const size_t plane_cells = (size_t)a.g.B * ((size_t)H * W);

    sft_cells<T>(RH, RW, [&](int r, int c) {
        const int y = ry + r, x = rx + c;
        const bool in = y >= 0 && y < H && x >= 0 && x < W;
        const size_t idx = p.base + (size_t)(in ? y * W + x : 0);
        C[r * RW + c] = in ? a.C[idx] : INF;      // (+inf: a cell outside the map stays +inf in every plane)
        prev[r * RW + c] = in ? a.src[idx] : INF;
    });
    __syncthreads();

    const uint32_t nm = a.nmask;
    for (int s = 1; s <= n; ++s) {
        const int k = a.k0 + s;
        // where this sweep's interior goes: out0 = the launch's result or the final slot, out1 = a checkpoint
        float* out0 = s == n ? a.dst : nullptr;
        float* out1 = nullptr;
        if (a.tape) {
            const int d = k - a.tape_k0;
            if (d >= a.tape_every && d % a.tape_every == 0 && d / a.tape_every <= a.tape_count) out1 = a.tape + (size_t)(d / a.tape_every - 1) * plane_cells;
            if (k == a.final_k) out0 = a.tape + (size_t)a.final_slot * plane_cells;
        }
        sft_cells<T>(RH - 2 * s, RW - 2 * s, [&](int r, int c) {
            const int lr = r + s, lc = c + s, i = lr * RW + lc;
            const int y = ry + lr, x = rx + lc;
            const float* at = prev + i;
            const SoftMin sm = sfl_softmin([&](int dy, int dx) { return at[dy * RW + dx]; }, nm, y > 0, y < H - 1, x > 0, x < W - 1);
            const float cc = C[i];
            const float v = cc < 0.f ? 0.f : sm.m < INF ? cc + (sm.m - sfl_log2(sm.s)) : INF;
            next[i] = v;
            if ((out0 || out1) && lr >= n && lr < n + p.rows && lc >= n && lc < n + p.cols) {
                const size_t idx = p.base + (size_t)(y * W + x);
                if (out0) out0[idx] = v;
                if (out1) out1[idx] = v;
            }
        });
        __syncthreads();
        float* t = prev;
        prev = next;
        next = t;
    }
    // prev is plane k0 + n on the interior, next plane k0 + n - 1 on the interior and one ring

    if (!a.last) return;
    const bool map_bad = a.flags[2 * p.b + 1] != 0;
    const size_t HW = (size_t)H * W;
    float* pol = a.policy ? a.policy + p.base * 8 : nullptr;
    float* lpol = LOGP ? log_policy + p.base * 8 : nullptr;
    sft_cells<T>(p.rows, p.cols, [&](int r, int c) {
        const int i = (r + n) * RW + (c + n);
        const int y = p.y0 + r, x = p.x0 + c;
        const size_t cell = (size_t)(y * W + x);
        a.dist[p.base + cell] = map_bad ? INF : a.goal[p.base + cell] != 0.f ? 0.f : prev[i] * a.from_units;
        if (LOGP || pol) {
            const bool up = y > 0, dn = y < H - 1, lf = x > 0, rt = x < W - 1;
            const float* at = next + i;
            const SoftMin sm = sfl_softmin([&](int dy, int dx) { return at[dy * RW + dx]; }, nm, up, dn, lf, rt);
            const float cc = C[i];
            const bool live = cc >= 0.f && cc < INF && sm.m < INF;
            float log2s = 0.f;
            if constexpr (LOGP) log2s = sfl_log2(sm.s);
            fld_each<8>([&](auto k) __attribute__((always_inline)) {
                constexpr Move mv = kActionMoves[decltype(k)::value];
                float w = 0.f, lw = -INF;
                if (live && (nm & fld_bit(mv.dy, mv.dx)) && fld_inside(mv.dy, mv.dx, up, dn, lf, rt)) {
                    w = sfl_exp2(sm.m - at[mv.dy * RW + mv.dx]) / sm.s;
                    // the minimum and the sum kept apart, as in w: -inf by itself for a target of +inf
                    if constexpr (LOGP) lw = ((sm.m - at[mv.dy * RW + mv.dx]) - log2s) * (float)M_LN2;
                }
                if (!LOGP || pol) pol[(size_t) decltype(k)::value * HW + cell] = w;
                if constexpr (LOGP) lpol[(size_t) decltype(k)::value * HW + cell] = lw;
            });
        }
    });
}


// A_K = the upstream gradient on the cells live at K (U is plane K), 0 elsewhere; the fp64 sums start there
// (POLICY: a.grad_dist may be nullptr = zeros)
template <int T, bool POLICY = false>
__global__ __launch_bounds__(T) void nastar_soft_tiled_grad_init_kernel(const SoftTileGradArgs a)
{
    const TilePos p = tld_pos(a.g);
    const int W = a.g.W;
    sft_cells<T>(p.rows, p.cols, [&](int r, int c) {
        const size_t idx = p.base + (size_t)((p.y0 + r) * W + (p.x0 + c));
        const float cc = a.C[idx];
        const bool live = cc >= 0.f && cc < INFINITY && a.U[idx] < INFINITY;  // passable, no goal, finite at K
        float g = 0.f;
        if (live && (!POLICY || a.grad_dist)) g = a.grad_dist[idx];
        a.A_out[idx] = g;
        a.sum[idx] = (double)g;
    });
}

// the second seed of the tiled backward (include/nastar_soft_policy_tiled.h): the upstream gradient of the log-policy [B,8,HW], and plane K,
// which says where a cell is live at K
struct SoftTilePolicySeed {
    const float* grad_log_policy;
    const float* UK;
    float neg_inv_tau;  // -1 / tau
};

// ONE STEP k of the backward on one tile.  INJECT (step K only, nastar_soft_policy_tiled.hip.h): the log-policy seed GL joins the gather,
// A_{K-1} = the gather + Z.  The first pass also leaves Q(n) = gsum(n) / S_K(n) and a byte "live at K" (from C and plane K) on the tile and
// one ring; the gather adds GL(a,n) - exp2(M(n) - u) Q(n) over the predecessors live at K: the statements of sfl_backward<T, true>.  Without
// it every statement is the plain step's, and `seed` is never looked at: the same instruction stream, the same bits.
template <int T, bool INJECT = false>
__global__ __launch_bounds__(T) void nastar_soft_tiled_grad_step_kernel(const SoftTileGradArgs a, const SoftTilePolicySeed seed)
{
    extern __shared__ __attribute__((aligned(16))) char sfg_tile_smem[];
    const TilePos p = tld_pos(a.g);
    const int H = a.g.H, W = a.g.W;
    const int UH = p.rows + 4, UW = p.cols + 4, PH = p.rows + 2, PW = p.cols + 2;
    float* U = reinterpret_cast<float*>(sfg_tile_smem);  // plane k - 1; its cell (0, 0) is the map's (y0 - 2, x0 - 2)
    float* P = U + UH * UW;                               // A_k, then P; its cell (0, 0) is the map's (y0 - 1, x0 - 1)
    float* M = P + PH * PW;
    float* Q = M + PH * PW;                               // (INJECT) as P
    uint8_t* liveK = reinterpret_cast<uint8_t*>(Q + PH * PW);
    const size_t HW = (size_t)H * W;
    const float* gl = INJECT ? seed.grad_log_policy + p.base * 8 : nullptr;
    const float INF = INFINITY;

    sft_cells<T>(UH, UW, [&](int r, int c) {
        const int y = p.y0 - 2 + r, x = p.x0 - 2 + c;
        const bool in = y >= 0 && y < H && x >= 0 && x < W;
        U[r * UW + c] = in ? a.U[p.base + (size_t)(in ? y * W + x : 0)] : INF;
    });
    sft_cells<T>(PH, PW, [&](int r, int c) {
        const int y = p.y0 - 1 + r, x = p.x0 - 1 + c;
        const bool in = y >= 0 && y < H && x >= 0 && x < W;
        P[r * PW + c] = in ? a.A_in[p.base + (size_t)(in ? y * W + x : 0)] : 0.f;
    });
    __syncthreads();

    const uint32_t nm = a.nmask;
    sft_cells<T>(PH, PW, [&](int r, int c) {
        const int y = p.y0 - 1 + r, x = p.x0 - 1 + c, i = r * PW + c;
        const float* at = U + (r + 1) * UW + (c + 1);
        const bool up = y > 0, dn = y < H - 1, lf = x > 0, rt = x < W - 1;
        const SoftMin sm = sfl_softmin([&](int dy, int dx) { return at[dy * UW + dx]; }, nm, up, dn, lf, rt);
        const bool any = sm.m < INF;  // (A is 0 on a cell that is not live at k, whatever its soft-min)
        P[i] = any ? P[i] / sm.s : 0.f;
        M[i] = any ? sm.m : -INF;     // exp2(-inf - u) = 0
        if constexpr (INJECT) {
            bool live = false;
            const size_t cell = (size_t)(y * W + x);  // (inside the map wherever it is used)
            if (y >= 0 && y < H && x >= 0 && x < W) {
                const float cc = a.C[p.base + cell];
                live = cc >= 0.f && cc < INF && seed.UK[p.base + cell] < INF;  // passable, no goal, finite at K: what the init kernel asks
            }
            float gsum = 0.f;
            if (live) {  // GL is read on Act(n) only, in the row-major order of the move offsets
                fld_each<8>([&](auto j) __attribute__((always_inline)) {
                    constexpr Move o = kChildOffsets[decltype(j)::value];
                    if ((nm & fld_bit(o.dy, o.dx)) && fld_inside(o.dy, o.dx, up, dn, lf, rt) && at[o.dy * UW + o.dx] < INF)
                        gsum += gl[(size_t)kOppositeAction[7 - decltype(j)::value] * HW + cell];
                });
            }
            Q[i] = gsum / sm.s;  // (S >= 1 on a live cell; what is not live is 0 / S or 0 / 0 and is never read)
            liveK[i] = live;
        }
    });
    __syncthreads();

    sft_cells<T>(p.rows, p.cols, [&](int r, int c) {
        const int y = p.y0 + r, x = p.x0 + c, i = (r + 1) * PW + (c + 1);
        const bool up = y > 0, dn = y < H - 1, lf = x > 0, rt = x < W - 1;
        const float u = U[(r + 2) * UW + (c + 2)];
        float acc = 0.f, z = 0.f;
        // the predecessor at kChildOffsets[j] steps onto this cell by the opposite move
        fld_each<8>([&](auto j) __attribute__((always_inline)) {
            constexpr Move o = kChildOffsets[decltype(j)::value];
            if ((nm & fld_bit(-o.dy, -o.dx)) && fld_inside(o.dy, o.dx, up, dn, lf, rt)) {
                const int n = i + o.dy * PW + o.dx;
                if constexpr (INJECT) {
                    const float w = sfl_exp2(M[n] - u);
                    acc += P[n] * w;
                    if (liveK[n] && u < INF)
                        z += gl[(size_t)kOppositeAction[decltype(j)::value] * HW + (size_t)((y + o.dy) * W + (x + o.dx))] - w * Q[n];
                } else {
                    acc += P[n] * sfl_exp2(M[n] - u);
                }
            }
        });
        const size_t idx = p.base + (size_t)(y * W + x);
        const float cc = a.C[idx];
        float v = acc;
        if constexpr (INJECT) v = acc + z * seed.neg_inv_tau;
        v = (cc >= 0.f && cc < INF && u < INF) ? v : 0.f;
        a.A_out[idx] = v;
        a.sum[idx] += (double)v;  // (INJECT: the sum is A_K alone until here)
    });
}


// one rounding per cell
template <int T>
__global__ __launch_bounds__(T) void nastar_soft_tiled_grad_store_kernel(const SoftTileGradArgs a)
{
    const TilePos p = tld_pos(a.g);
    const int W = a.g.W;
    const bool map_bad = a.flags[2 * p.b + 1] != 0;
    sft_cells<T>(p.rows, p.cols, [&](int r, int c) {
        const size_t idx = p.base + (size_t)((p.y0 + r) * W + (p.x0 + c));
        a.grad_cost[idx] = map_bad ? 0.f : (float)a.sum[idx];
    });
}

}  // namespace nastar
