// nastar_fields_grad.hip.h -- the gradient of the cost-to-go field with respect to the cost maps: a subtree sum over the policy forest
// (include/nastar_fields_grad.h).
//
// One workgroup owns one map, as in nastar_fields.hip.h, and a lane owns the cells tid, tid + T, ... -- at most kGradCellsPerLane of them, so
// that what a lane knows about ITS cells stays in registers.  LDS holds
//   A[i]     fp64, 8 B per cell: the subtree sum of a live cell.  (Before the loop the same bytes hold the readable field as fp32.)
//   succ[i]  one byte per cell: the action a live cell takes, 0xFF for "none" and on cells that are not live;
//   flags    the three sweep flags of fld_sweep, then has_live [3] and plateau [4].
// Set-up, three barriers: the readable field; every live cell's successor (fld_best_action: the forward kernel's policy, on the same
// values) and, from the successors of its eight neighbours, the 8-bit set of its CHILDREN (fld_child_set).  After that neither dist nor
// succ is looked at again.  All three rules, and the loop, are those of nastar_field_rules.hip.h.
//
// A sweep recomputes, IN PLACE, every cell that has a child (fld_subtree_sum).  A cell without a child is final from the start (A = G).  A
// cell is a pure function of its children's values, the forest has no cycle (a successor has a strictly smaller dist), so there is ONE
// fixed point and its bits do not depend on the order of the updates or on what a racing read returned along the way: only the number of
// sweeps does.  A cell h edges above its deepest leaf is final after h sweeps at the latest; a sweep that changed no BITS read final values
// only.  Live cells <= H*W - 1, hence h <= H*W - 2 and the quiet sweep is at most number H*W - 1: the bound H*W is never hit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nastar_fields_grad.h"
#include "nastar_fields.hip.h"

namespace nastar {

constexpr int kFieldsGradMaxCells = kFieldsMaxCells;
constexpr int kGradCellsPerLane = kFieldCellsPerLane;

struct FieldGradArgs {
    const float* dist;       // [B,HW]
    const float* goal;
    const float* passable;
    const float* grad_dist;
    float* grad_cost;        // [B,HW]
    int32_t* status;         // [B]
    int32_t* sweeps;         // [B] or nullptr
    int H, W;
    uint32_t nmask;
};

// LDS bytes of one map: A, succ, then the flags
constexpr size_t fields_grad_lds_bytes(int HW) { return (size_t)HW * 8 + ((size_t)HW + 15) / 16 * 16 + 32; }

template <int T>
__global__ __launch_bounds__(T) void nastar_fields_backward_kernel(const FieldGradArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char fgr_smem[];
    constexpr int K = kGradCellsPerLane;
    constexpr uint8_t NONE = 0xFF;
    const int H = a.H, W = a.W, HW = H * W;  // HW <= K * T: the host picks T
    double* A = reinterpret_cast<double*>(fgr_smem);
    float* R = reinterpret_cast<float*>(fgr_smem);  // the readable field, until A takes the bytes over
    uint8_t* succ = reinterpret_cast<uint8_t*>(fgr_smem + (size_t)HW * 8);
    int* flags = reinterpret_cast<int*>(fgr_smem + (size_t)HW * 8 + ((size_t)HW + 15) / 16 * 16);
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * HW;
    const float INF = INFINITY;

    if (tid < 8) flags[tid] = 0;

    // ---- the readable field; what this lane keeps of its cells: dist, and (bit k of `live`) whether cell k is live ------------------------------
    float d[K];
    uint32_t live = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int i = tid + k * T;
        d[k] = INF;
        if (i < HW) {
            d[k] = a.dist[base + i];
            R[i] = a.passable[base + i] != 0.f ? d[k] : INF;
            if (a.goal[base + i] == 0.f && d[k] < INF) live |= 1u << k;  // (a NaN is not below +inf: not live)
        }
    }
    __syncthreads();

    // ---- successors ---------------------------------------------------------------------------------------------------------------------------
    const uint32_t nm = a.nmask;
    bool stuck = false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int i = tid + k * T;
        if (i < HW) {
            int best = -1;
            if (live >> k & 1) {
                const int r = i / W, c = i - r * W;
                best = fld_best_action([&](int dy, int dx) { return R[i + dy * W + dx]; }, nm, r > 0, r < H - 1, c > 0, c < W - 1, d[k]);
                stuck |= best < 0;
            }
            succ[i] = best < 0 ? NONE : (uint8_t)best;
        }
    }
    if (__ballot(live != 0) && (tid & 63) == 0) __hip_atomic_store(&flags[3], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (__ballot(stuck) && (tid & 63) == 0) __hip_atomic_store(&flags[4], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();  // (behind it nobody reads R any more: A may be written)
    const bool plateau = flags[4] != 0, any_live = flags[3] != 0;

    // ---- children, G, and A = G --------------------------------------------------------------------------------------------------------------
    float g[K];
    uint32_t kids[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int i = tid + k * T;
        g[k] = 0.f;
        kids[k] = 0;
        if ((live >> k & 1) && !plateau) {
            const int r = i / W, c = i - r * W;
            kids[k] = fld_child_set([&](int dy, int dx) { return succ[i + dy * W + dx]; }, r > 0, r < H - 1, c > 0, c < W - 1);
            g[k] = a.grad_dist[base + i];
            A[i] = (double)g[k];
        }
    }
    __syncthreads();

    // ---- accumulation ------------------------------------------------------------------------------------------------------------------------
    Sweeps run{0, true};
    if (any_live && !plateau) {
        run = fld_sweep(flags, HW, [&](bool backwards) {
            bool changed = false;
            if (!backwards) {
#pragma unroll
                for (int k = 0; k < K; ++k) changed |= fld_subtree_sum(A + tid + k * T, W, kids[k], g[k]);
            } else {
#pragma unroll
                for (int k = K - 1; k >= 0; --k) changed |= fld_subtree_sum(A + tid + k * T, W, kids[k], g[k]);
            }
            return changed;
        });
    }
    const bool quiet = run.quiet;

    // ---- epilogue: one rounding per live cell, zeros elsewhere; a map that did not converge has no gradient to show ------------------------------
    if (tid == 0) {
        a.status[blockIdx.x] = plateau ? NASTAR_ERR_PLATEAU : quiet ? NASTAR_OK : NASTAR_ERR_NO_CONVERGENCE;
        if (a.sweeps) a.sweeps[blockIdx.x] = run.sweeps;
    }
    const bool write_sums = !plateau && quiet;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int i = tid + k * T;
        if (i < HW) a.grad_cost[base + i] = (write_sums && (live >> k & 1)) ? (float)A[i] : 0.f;
    }
}

}  // namespace nastar
