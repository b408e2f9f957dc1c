// nastar_fields_grad.hip.h -- the gradient of the cost-to-go field with respect to the cost maps: a subtree sum over the policy forest
// (include/nastar_fields_grad.h).
//
// One workgroup owns one map, as in nastar_fields.hip.h, and a lane owns the cells tid, tid + T, ... -- at most kGradCellsPerLane of them, so
// that what a lane knows about ITS cells stays in registers.  LDS holds
//   A[i]     fp64, 8 B per cell: the subtree sum of a live cell.  (Before the loop the same bytes hold the readable field as fp32.)
//   succ[i]  one byte per cell: the action a live cell takes, 0xFF for "none" and on cells that are not live;
//   flags    the three sweep flags in rotation (nastar_fields.hip.h), then has_live [3] and plateau [4].
// Set-up, three barriers: the readable field; every live cell's successor (the forward kernel's policy, on the same values) and, from the
// successors of its eight neighbours, the 8-bit set of its CHILDREN -- bit k = the neighbour at kGradChild[k] steps onto this cell.  After
// that neither dist nor succ is looked at again.
//
// A sweep recomputes, IN PLACE, every cell that has a child: A(v) = G(v) + A(c_0) + A(c_1) + ... in fp64, the children in the one order of
// the header.  A cell without a child is final from the start (A = G).  A cell is a pure function of its children's values, the forest has
// no cycle (a successor has a strictly smaller dist), so there is ONE fixed point and its bits do not depend on the order of the updates or
// on what a racing read returned along the way: only the number of sweeps does.  (A is read and written through relaxed workgroup-scope
// 64-bit atomics: ds_read_b64 / ds_write_b64, no data race in the language's sense.)  A cell h edges above its deepest leaf is final after
// h sweeps at the latest; a sweep that changed no BITS (bits, so that a NaN in G on a live cell is a value like any other) read final values
// only.  Live cells <= H*W - 1, hence h <= H*W - 2 and the quiet sweep is at most number H*W - 1: the bound H*W is never hit.  Even sweeps
// visit a lane's cells upwards, odd sweeps downwards, as the forward kernel does: a lane's later visit reads what its earlier one wrote.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nastar_fields_grad.h"
#include "nastar_fields.hip.h"

namespace nastar {

constexpr int kFieldsGradMaxCells = kFieldsMaxCells;
constexpr int kGradCellsPerLane = 16;  // 64 lanes x 16 = 1024 cells, 256 x 16 = 4096, 1024 x 16 = 16384

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

__device__ __forceinline__ double fgr_load(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void fgr_store(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

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

    // ---- successors: the policy of nastar_fields.hip.h ---------------------------------------------------------------------------------------
    const uint32_t nm = a.nmask;
    bool stuck = false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int i = tid + k * T;
        if (i < HW) {
            int best = -1;
            if (live >> k & 1) {
                const int r = i / W, c = i - r * W;
                const bool up = r > 0, dn = r < H - 1, lf = c > 0, rt = c < W - 1;
                float m = INF;
                // synthetic.ACTION_MOVES order; a strict < keeps the first action among equals
#define NASTAR_FGR_ACT(act, dy, dx, ok)                                          \
    if ((nm & fld_bit(dy, dx)) && (ok)) {                                         \
        const float v = R[i + (dy) * W + (dx)];                                   \
        if (v < m) {                                                              \
            m = v;                                                                \
            best = act;                                                           \
        }                                                                         \
    }
                NASTAR_FGR_ACT(0, -1, 0, up)
                NASTAR_FGR_ACT(1, 0, 1, rt)
                NASTAR_FGR_ACT(2, 0, -1, lf)
                NASTAR_FGR_ACT(3, 1, 0, dn)
                NASTAR_FGR_ACT(4, -1, 1, up && rt)
                NASTAR_FGR_ACT(5, -1, -1, up && lf)
                NASTAR_FGR_ACT(6, 1, 1, dn && rt)
                NASTAR_FGR_ACT(7, 1, -1, dn && lf)
#undef NASTAR_FGR_ACT
                if (!(m < d[k])) best = -1;
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
    uint32_t kids[K];  // bit j: the neighbour at the j-th offset of the header's order is a child (its action is the opposite move)
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int i = tid + k * T;
        g[k] = 0.f;
        kids[k] = 0;
        if ((live >> k & 1) && !plateau) {
            const int r = i / W, c = i - r * W;
            const bool up = r > 0, dn = r < H - 1, lf = c > 0, rt = c < W - 1;
            uint32_t m = 0;
            // the neighbour at (dy, dx) steps onto this cell by the move (-dy, -dx): action `act` of ACTION_MOVES
#define NASTAR_FGR_KID(j, dy, dx, ok, act) \
    if ((ok) && succ[i + (dy) * W + (dx)] == (act)) m |= 1u << (j);
            NASTAR_FGR_KID(0, -1, -1, up && lf, 6)
            NASTAR_FGR_KID(1, -1, 0, up, 3)
            NASTAR_FGR_KID(2, -1, 1, up && rt, 7)
            NASTAR_FGR_KID(3, 0, -1, lf, 1)
            NASTAR_FGR_KID(4, 0, 1, rt, 2)
            NASTAR_FGR_KID(5, 1, -1, dn && lf, 4)
            NASTAR_FGR_KID(6, 1, 0, dn, 0)
            NASTAR_FGR_KID(7, 1, 1, dn && rt, 5)
#undef NASTAR_FGR_KID
            kids[k] = m;
            g[k] = a.grad_dist[base + i];
            A[i] = (double)g[k];
        }
    }
    __syncthreads();

    // ---- accumulation ------------------------------------------------------------------------------------------------------------------------
    int sweeps = 0;
    bool quiet = true;
    if (any_live && !plateau) {
        quiet = false;
        for (int s = 0; s < HW; ++s) {  // the bound: no input moves it
            bool changed = false;
            auto visit = [&](int k) {
                const uint32_t m = kids[k];
                if (m) {
                    double* p = A + tid + k * T;
                    double v = (double)g[k];
#define NASTAR_FGR_ADD(j, dy, dx) \
    if (m & (1u << (j))) v += fgr_load(p + (dy) * W + (dx));
                    NASTAR_FGR_ADD(0, -1, -1)
                    NASTAR_FGR_ADD(1, -1, 0)
                    NASTAR_FGR_ADD(2, -1, 1)
                    NASTAR_FGR_ADD(3, 0, -1)
                    NASTAR_FGR_ADD(4, 0, 1)
                    NASTAR_FGR_ADD(5, 1, -1)
                    NASTAR_FGR_ADD(6, 1, 0)
                    NASTAR_FGR_ADD(7, 1, 1)
#undef NASTAR_FGR_ADD
                    if (__double_as_longlong(v) != __double_as_longlong(fgr_load(p))) {
                        fgr_store(p, v);
                        changed = true;
                    }
                }
            };
            if ((s & 1) == 0) {
#pragma unroll
                for (int k = 0; k < K; ++k) visit(k);
            } else {
#pragma unroll
                for (int k = K - 1; k >= 0; --k) visit(k);
            }
            const int slot = s % 3;
            if (__ballot(changed) && (tid & 63) == 0) __hip_atomic_store(&flags[slot], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (tid == 0) __hip_atomic_store(&flags[slot == 2 ? 0 : slot + 1], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __syncthreads();
            ++sweeps;
            if (__hip_atomic_load(&flags[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0) {
                quiet = true;
                break;
            }
        }
    }

    // ---- epilogue: one rounding per live cell, zeros elsewhere; a map that did not converge has no gradient to show ------------------------------
    if (tid == 0) {
        a.status[blockIdx.x] = plateau ? NASTAR_ERR_PLATEAU : quiet ? NASTAR_OK : NASTAR_ERR_NO_CONVERGENCE;
        if (a.sweeps) a.sweeps[blockIdx.x] = sweeps;
    }
    const bool write_sums = !plateau && quiet;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int i = tid + k * T;
        if (i < HW) a.grad_cost[base + i] = (write_sums && (live >> k & 1)) ? (float)A[i] : 0.f;
    }
}

}  // namespace nastar
