// nastar_path_masks.hip.h -- the exact shortest path of every map as a 0/1 mask and its blackbox gradient with respect to the costs, one
// launch each (include/nastar_path_masks.h).
//
// One workgroup owns one map, with the LDS plan of nastar_fields.hip.h: R[i], the field as the relaxation reads it, and C[i], the cost with
// the obstacles folded in as +inf.  Four steps:
//   (a) load (the backward instantiation perturbs the cost on the way) and relax to the fixed point: the load rule, the relaxation of a
//       cell and fld_sweep are those of nastar_cost_to_go_kernel, so R holds the same bits;
//   (b) lane 0 chases from the start with fld_best_action on R -- the successor of nastar_field_routes.hip.h: for every cell a move may
//       enter, R IS the readable field -- under the unconditional bound of H*W hops, and MARKS every route cell in C, which nobody reads
//       after the last sweep's barrier.  The mark is -1: a cost in C is >= 0, +inf or (on a map that is never chased) a NaN, never below 0.
//       A cell with R > 0 is no goal, so goal[] is read from memory once per chase: where R is 0;
//   (c) behind ONE barrier all lanes store the map's row from C, a cell per lane and round, coalesced.  This pass alone writes the output:
//       no two lanes ever store to one address;
//   (d) lane 0 writes the status and the field at the start.
// No workgroup waits for another.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nastar_path_masks.h"
#include "nastar_fields.hip.h"

namespace nastar {

constexpr int kPathMasksMaxCells = kFieldsMaxCells;
constexpr float kPathMark = -1.f;

struct PathMaskArgs {
    const float* cost;          // [B,HW]
    const float* goal;
    const float* passable;
    const int32_t* start;       // [B]
    const float* grad_path;     // [B,HW]   (backward)
    const float* path_fwd;      // [B,HW]   (backward)
    const int32_t* status_fwd;  // [B]      (backward)
    float* out;                 // [B,HW]: the mask, or the gradient
    float* path_cost;           // [B] or nullptr (forward)
    int32_t* status;            // [B]; may be nullptr in the backward call
    float lambda, inv_lambda, min_cost;
    int H, W;
    uint32_t nmask;
    int vec;                    // every map-sized input pointer is 16-byte aligned: float4 loads between a scalar head and a scalar tail
};

// the perturbed cost: two separately rounded operations and the clamp; a NaN stays one (fmaxf alone would return min_cost)
__device__ __forceinline__ float pmk_perturbed(float c, float g, float lambda, float min_cost)
{
    const float s = __fadd_rn(__fmul_rn(lambda, g), c);
    return s != s ? s : fmaxf(s, min_cost);
}

template <int T, bool kBackward>
__global__ __launch_bounds__(T) void nastar_path_masks_kernel(const PathMaskArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char pmk_smem[];
    const int H = a.H, W = a.W, HW = H * W;
    float* R = reinterpret_cast<float*>(pmk_smem);
    float* C = R + HW;
    int* flags = reinterpret_cast<int*>(pmk_smem + ((size_t)HW * 8 + 15) / 16 * 16);  // [0..2] sweep flags, [3] has_goal, [4] bad_cost, [5] chase status
    const int tid = threadIdx.x;
    const size_t map = blockIdx.x, base = map * (size_t)HW;
    const float* cost = a.cost + base;
    const float* goal = a.goal + base;
    const float* pass = a.passable + base;
    float* out = a.out + base;
    const float INF = INFINITY;

    if constexpr (kBackward) {
        if (a.status_fwd[map] != NASTAR_OK) {  // (the same word for every lane) the forward gave no path: no gradient, nothing to solve
            for (int i = tid; i < HW; i += T) out[i] = 0.f;
            if (tid == 0 && a.status) a.status[map] = NASTAR_OK;
            return;
        }
    }

    if (tid < 8) flags[tid] = 0;
    __syncthreads();

    // ---- (a) load: the rule of nastar_cost_to_go_kernel, on the perturbed cost in the backward call ------------------------------------------
    const float* gpath = kBackward ? a.grad_path + base : nullptr;
    const float lambda = a.lambda, min_cost = a.min_cost;
    bool has_goal = false, bad = false;
    auto cell = [&](int i, float c, float g, float p) {
        const bool ok = p != 0.f;
        bad |= ok && !(c >= 0.f);
        has_goal |= g != 0.f;
        C[i] = ok ? c : INF;
        R[i] = (ok && g != 0.f) ? 0.f : INF;
    };
    int head = HW, nvec = 0;
    if (a.vec) {
        head = (int)((4 - (base & 3)) & 3);
        if (head > HW) head = HW;
        nvec = (HW - head) >> 2;
    }
    for (int v = tid; v < nvec; v += T) {
        const int i = head + 4 * v;
        float4 c = *reinterpret_cast<const float4*>(cost + i);
        const float4 g = *reinterpret_cast<const float4*>(goal + i);
        const float4 p = *reinterpret_cast<const float4*>(pass + i);
        if constexpr (kBackward) {
            const float4 q = *reinterpret_cast<const float4*>(gpath + i);
            c.x = pmk_perturbed(c.x, q.x, lambda, min_cost);
            c.y = pmk_perturbed(c.y, q.y, lambda, min_cost);
            c.z = pmk_perturbed(c.z, q.z, lambda, min_cost);
            c.w = pmk_perturbed(c.w, q.w, lambda, min_cost);
        }
        cell(i, c.x, g.x, p.x);
        cell(i + 1, c.y, g.y, p.y);
        cell(i + 2, c.z, g.z, p.z);
        cell(i + 3, c.w, g.w, p.w);
    }
    const int tail0 = head + 4 * nvec, nscalar = head + (HW - tail0);
    for (int k = tid; k < nscalar; k += T) {
        const int i = k < head ? k : tail0 + (k - head);
        float c = cost[i];
        if constexpr (kBackward) c = pmk_perturbed(c, gpath[i], lambda, min_cost);
        cell(i, c, goal[i], pass[i]);
    }
    if (__ballot(has_goal) && (tid & 63) == 0) __hip_atomic_store(&flags[3], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (__ballot(bad) && (tid & 63) == 0) __hip_atomic_store(&flags[4], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    const bool map_bad = flags[4] != 0, map_goal = flags[3] != 0;
    const int n0 = a.start[map];
    const bool inside = n0 >= 0 && n0 < HW;

    // ---- (a) relaxation: the cell rule and the sweep order of nastar_cost_to_go_kernel ------------------------------------------------------------
    const uint32_t nm = a.nmask;
    Sweeps run{0, true};
    if (inside && !map_bad && map_goal) {
        const int r0 = tid / W, c0 = tid - r0 * W;
        const int dr = T / W, dc = T - dr * W;
        const int ilast = tid < HW ? tid + (HW - 1 - tid) / T * T : 0;
        const int rl = ilast / W, cl = ilast - rl * W;
        bool changed;
        auto relax = [&](int i, int r, int c) {
            const bool up = r > 0, dn = r < H - 1, lf = c > 0, rt = c < W - 1;
            float m = INF;
            fld_each<8>([&](auto j) __attribute__((always_inline)) {
                constexpr Move o = kChildOffsets[decltype(j)::value];
                if (nm & fld_bit(o.dy, o.dx)) m = fminf(m, fld_inside(o.dy, o.dx, up, dn, lf, rt) ? fld_load(R + i + o.dy * W + o.dx) : INF);
            });
            const float cand = C[i] + m;
            if (cand < fld_load(R + i)) {
                fld_store(R + i, cand);
                changed = true;
            }
        };
        run = fld_sweep(flags, HW, [&](bool backwards) {
            changed = false;
            if (!backwards) {
                int r = r0, c = c0;
                for (int i = tid; i < HW; i += T) {
                    relax(i, r, c);
                    r += dr;
                    c += dc;
                    if (c >= W) {
                        c -= W;
                        ++r;
                    }
                }
            } else {
                int r = rl, c = cl;
                for (int i = ilast; i >= tid && tid < HW; i -= T) {
                    relax(i, r, c);
                    r -= dr;
                    c -= dc;
                    if (c < 0) {
                        c += W;
                        --r;
                    }
                }
            }
            return changed;
        });
    }

    // ---- (b) the chase: one lane; (d) its verdict and the field at the start -----------------------------------------------------------------------
    if (tid == 0) {
        int st = !inside ? NASTAR_ERR_BAD_SHAPE : map_bad ? NASTAR_ERR_BAD_COST : !map_goal ? NASTAR_ERR_UNSOLVABLE : NASTAR_OK;
        float d0 = INF;
        if (st == NASTAR_OK) {
            d0 = goal[n0] != 0.f ? 0.f : R[n0];  // a goal cell holds 0, passable or not
            if (!(d0 < INF)) st = NASTAR_ERR_UNSOLVABLE;
            else if (!run.quiet) st = NASTAR_ERR_NO_CONVERGENCE;
        }
        if (st == NASTAR_OK) {
            st = NASTAR_ERR_PLATEAU;
            int n = n0, y = n0 / W, x = n0 - y * W;
            float d = d0;
            for (int hop = 0; hop < HW; ++hop) {  // the bound: no input moves it (s strictly lowers the field)
                C[n] = kPathMark;
                if (d == 0.f) {  // a goal, or a zero-cost plateau: nothing is below 0
                    if (goal[n] != 0.f) st = NASTAR_OK;
                    break;
                }
                const int best = fld_best_action([&](int dy, int dx) { return R[n + dy * W + dx]; }, nm, y > 0, y < H - 1, x > 0, x < W - 1, d);
                if (best < 0) break;
                const Move mv = fld_move<kActionMoves>(best);
                y += mv.dy;
                x += mv.dx;
                n += mv.dy * W + mv.dx;
                d = R[n];
            }
        }
        flags[5] = st;
        if (a.status) a.status[map] = st;
        if (!kBackward && a.path_cost) a.path_cost[map] = st == NASTAR_OK ? d0 : INF;
    }
    __syncthreads();

    // ---- (c) the row: every cell of the output, by this pass alone -------------------------------------------------------------------------------------
    const bool found = flags[5] == NASTAR_OK;
    if constexpr (kBackward) {
        const float* fwd = a.path_fwd + base;
        const float inv_lambda = a.inv_lambda;
        for (int i = tid; i < HW; i += T) out[i] = found ? ((C[i] < 0.f ? 1.f : 0.f) - fwd[i]) * inv_lambda : NAN;
    } else {
        for (int i = tid; i < HW; i += T) out[i] = (found && C[i] < 0.f) ? 1.f : 0.f;
    }
}

}  // namespace nastar
