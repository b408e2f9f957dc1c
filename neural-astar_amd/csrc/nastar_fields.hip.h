// nastar_fields.hip.h -- the cost-to-go field of whole maps and its optimal policy (include/nastar_fields.h).
//
// One workgroup owns one map.  LDS holds two fp32 per cell for the whole computation:
//   R[i]  the field as the RELAXATION reads it: 0 on passable goals, +inf elsewhere at the start, only ever lowered.  An obstacle stays +inf
//         -- also a goal on an obstacle, which no move may enter; its 0 is written by the epilogue alone;
//   C[i]  the cost with the obstacles folded in as +inf, so that the loop has no passable test: fl32(+inf + x) never lowers anything.
// A passable goal needs no test either: its candidate fl32(c + x) >= 0 is never below its 0.
//
// A sweep relaxes every cell once, IN PLACE: R[i] = min(R[i], fl32(C[i] + min over the allowed moves i -> m of R[m])).  Because
// x -> fl32(c + x) is monotone, min over m of fl32(c + R[m]) == fl32(c + min over m of R[m]) -- one addition per cell -- and every value a lane
// can read, fresh or stale, is an upper bound of the fixed point, so the order of the updates changes the number of sweeps and never the
// result.  (R is read and written through relaxed workgroup-scope atomics: plain ds_read_b32 / ds_write_b32, and no data race in the
// language's sense.)  A sweep that lowered nothing read final values only: the fixed point -- fld_sweep (nastar_field_rules.hip.h) owns the
// loop and its detection.  The trip count is bounded by H*W whatever the data: a shortest route has fewer than H*W hops, and every sweep
// settles one more hop.  The policy is fld_best_action of the same header.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nastar_fields.h"
#include "nastar_field_rules.hip.h"

namespace nastar {

constexpr int kFieldsMaxCells = 16384;  // 2 x 4 B x 16384 = 128 KiB of the 160 KiB a workgroup may own

struct FieldArgs {
    const float* cost;      // [B,HW]
    const float* goal;
    const float* passable;
    float* dist;            // [B,HW]
    float* policy;          // [B,8,HW] or nullptr
    int32_t* status;        // [B]
    int32_t* sweeps;        // [B] or nullptr
    int H, W;
    uint32_t nmask;
    int vec;                // the three input pointers are 16-byte aligned: float4 loads between a scalar head and a scalar tail
};

// LDS bytes of one map: R, C, then the flags (16 bytes: has_goal, bad_cost are [3], [4] behind the three sweep flags)
inline size_t fields_lds_bytes(int HW) { return ((size_t)HW * 8 + 15) / 16 * 16 + 32; }

__device__ __forceinline__ float fld_load(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void fld_store(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

template <int T>
__global__ __launch_bounds__(T) void nastar_cost_to_go_kernel(const FieldArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char fld_smem[];
    const int H = a.H, W = a.W, HW = H * W;
    float* R = reinterpret_cast<float*>(fld_smem);
    float* C = R + HW;
    int* flags = reinterpret_cast<int*>(fld_smem + ((size_t)HW * 8 + 15) / 16 * 16);  // [0..2] sweep flags, [3] has_goal, [4] bad_cost
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * HW;
    const float* cost = a.cost + base;
    const float* goal = a.goal + base;
    const float* pass = a.passable + base;
    const float INF = INFINITY;

    if (tid < 8) flags[tid] = 0;
    __syncthreads();

    // ---- load: once, float4 where the addresses allow it ------------------------------------------------------------------------------------
    bool has_goal = false, bad = false;
    auto cell = [&](int i, float c, float g, float p) {
        const bool ok = p != 0.f;
        bad |= ok && !(c >= 0.f);                 // NaN or negative on a passable cell (-0.0 >= 0)
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
        const float4 c = *reinterpret_cast<const float4*>(cost + i);
        const float4 g = *reinterpret_cast<const float4*>(goal + i);
        const float4 p = *reinterpret_cast<const float4*>(pass + i);
        cell(i, c.x, g.x, p.x);
        cell(i + 1, c.y, g.y, p.y);
        cell(i + 2, c.z, g.z, p.z);
        cell(i + 3, c.w, g.w, p.w);
    }
    const int tail0 = head + 4 * nvec, nscalar = head + (HW - tail0);
    for (int k = tid; k < nscalar; k += T) {
        const int i = k < head ? k : tail0 + (k - head);
        cell(i, cost[i], goal[i], pass[i]);
    }
    if (__ballot(has_goal) && (tid & 63) == 0) __hip_atomic_store(&flags[3], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (__ballot(bad) && (tid & 63) == 0) __hip_atomic_store(&flags[4], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    const bool map_bad = flags[4] != 0, map_goal = flags[3] != 0;

    // ---- relaxation ---------------------------------------------------------------------------------------------------------------------------
    const uint32_t nm = a.nmask;
    const int r0 = tid / W, c0 = tid - r0 * W;    // the cell of this lane in the first round; round k + 1 is T cells on
    const int dr = T / W, dc = T - dr * W;
    Sweeps run{0, true};
    if (!map_bad && map_goal) {
        // the last cell of this lane, for the sweeps that run backwards
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
        // forward sweeps run down the map, backward sweeps up: a round reads what the round before it wrote, so values travel many rows per
        // sweep in the direction of the sweep and one row against it
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

    // ---- epilogue: the field, then the policy planes, every store coalesced ---------------------------------------------------------------------
    if (tid == 0) {
        a.status[blockIdx.x] = map_bad ? NASTAR_ERR_BAD_COST : !map_goal ? NASTAR_ERR_UNSOLVABLE : run.quiet ? NASTAR_OK : NASTAR_ERR_NO_CONVERGENCE;
        if (a.sweeps) a.sweeps[blockIdx.x] = run.sweeps;
    }
    float* dist = a.dist + base;
    for (int i = tid; i < HW; i += T) dist[i] = map_bad ? INF : (goal[i] != 0.f ? 0.f : R[i]);
    if (a.policy) {
        float* pol = a.policy + base * 8;
        int r = r0, c = c0;
        for (int i = tid; i < HW; i += T) {
            const float d = map_bad ? INF : R[i];
            int best = -1;
            if (d > 0.f && d < INF)
                best = fld_best_action([&](int dy, int dx) { return R[i + dy * W + dx]; }, nm, r > 0, r < H - 1, c > 0, c < W - 1, d);
#pragma unroll
            for (int k = 0; k < 8; ++k) pol[(size_t)k * HW + i] = (k == best) ? 1.f : 0.f;
            r += dr;
            c += dc;
            if (c >= W) {
                c -= W;
                ++r;
            }
        }
    }
}

}  // namespace nastar
