// nastar_soft_routes.hip.h -- sampled routes from the maximum-entropy route distribution of the soft field: N draws for each of S start
// cells per map, with lengths, costs, log-probabilities and visit counts (include/nastar_soft_routes.h).
//
// One move of the walker of one lane is written ONCE (`srt_move` below): it reads the eight values of plane K-j-1 around its cell, forms the
// weights, draws and moves.  Where the plane comes from is the kernel's compile-time switch:
//   LDS      a workgroup of T lanes serves one map and T of its walkers.  All walkers of a map read the same plane at the same move, so the
//            workgroup streams the tape BACKWARDS through LDS, one plane per move, double-buffered: the loads of plane K-j-2 are issued into
//            registers before the step of move j, which gathers from plane K-j-1 in LDS (Philox and the draw run in the loads' shadow), and
//            are written to the other buffer behind it; one barrier per move, which also counts the walkers still on their way -- the
//            workgroup stops when none is.  A byte per cell holds "goal" and "passable goal" (the implicit plane V_0).
//   gather   each lane reads its eight values from the tape in global memory: one dependent round trip per move, no barrier, nothing
//            streamed.  A wavefront ends with its last walker.
// Both give the same bits: the step is the same statements.  The slices of a map's walkers are independent workgroups: none waits for another.
// A walk that may outgrow its row (route_cap < K + 1) runs twice, first for the length, then for the stores -- the draw is a pure function
// of (seed, q, i, j), so the replay is the same walk.  The -1 of the rows and the zeros of the visit counts are a launch of their own in
// front (nastar_soft_routes_clear_kernel).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/nastar_soft_routes.h"
#include "nastar_field_rules.hip.h"
#include "nastar_soft_fields.hip.h"

namespace nastar {

constexpr int kSoftRoutesMaxCells = kSoftFieldsMaxCells;
constexpr int kSoftRoutesGatherT = 256;  // the width of the gather kernel's workgroups

struct SoftRoutesArgs {
    const float* cost;      // [B,HW]
    const float* goal;
    const float* passable;
    const float* tape;      // [B,K,HW]: plane k is tape + (k - 1) * HW, in units of tau ln 2
    const int32_t* start;   // [B,S]
    const float* uniforms;  // [B,S,N,K] or nullptr
    int32_t* routes;        // [B,S,N,cap] or nullptr
    int32_t* len;           // [B,S,N]
    float* route_cost;      // [B,S,N] or nullptr
    float* log_prob;        // [B,S,N] or nullptr
    int32_t* visits;        // [B,S,HW] or nullptr
    int32_t* status;        // [B,S]
    int groups;             // workgroups per map
    int S, N, H, W, K, cap;
    uint32_t nmask;
    uint32_t key0, key1;    // seed & 0xffffffff, seed >> 32
};

// floats between the two planes of the LDS kernel, and its LDS bytes: two planes, the goal bytes, the flags (bad_cost [1]); the gather
// kernel keeps the flags only
constexpr size_t srt_plane_stride(int HW) { return sfl_pad16((size_t)HW * 4) / 4; }
constexpr size_t soft_routes_lds_bytes(int HW, bool lds) { return lds ? 2 * sfl_pad16((size_t)HW * 4) + sfl_pad16((size_t)HW) + 32 : 32; }

// the first word of Philox4x32-10 of the counter (c0, c1, c2, c3) under the key (k0, k1)
__device__ __forceinline__ uint32_t srt_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0;
        c1 = lo1;
        c2 = n2;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

// in front of the walkers: routes[0, n_routes) = -1, visits[0, n_visits) = 0 (either may be empty); a grid-stride loop, coalesced stores
constexpr int kSoftRoutesClearT = 256;
template <int T>
__global__ __launch_bounds__(T) void nastar_soft_routes_clear_kernel(int32_t* routes, size_t n_routes, int32_t* visits, size_t n_visits)
{
    const size_t first = (size_t)blockIdx.x * T + threadIdx.x, stride = (size_t)gridDim.x * T;
    for (size_t i = first; i < n_routes; i += stride) routes[i] = -1;
    for (size_t i = first; i < n_visits; i += stride) visits[i] = 0;
}

// the walker of one lane between two moves
struct SrtWalker {
    int n, r, c, len;   // the cell it stands on, as an index and as (row, column); the route cells so far
    bool active;        // still on its way
    double csum, lsum;  // the fp64 tallies of route_cost and log_prob
};

// ONE MOVE of one walker that is still on its way, written ONCE for every kernel that walks (the two shapes below and the walker of
// nastar_soft_routes_tiled.hip.h): move j of walker (q, i), `row` its number in the batch.  value(m, is_goal&) -> U_{K-j-1}(m) is where the
// kernels differ: the plane the move reads, in LDS or in device memory.  The eight reads, the draw, the move, the tallies.  kFirst: the pass
// that tallies costs, log-probabilities and visits; visit(cell, l) sees route cell l.
template <bool kFirst, typename Value, typename Visit>
__device__ __forceinline__ void srt_move(const SoftRoutesArgs& a, const float* cost, SrtWalker& w, int j, int i, size_t q, size_t row,
                                         Value&& value, Visit&& visit)
{
    const int H = a.H, W = a.W, n = w.n;
    const float INF = INFINITY;
    const uint32_t nm = a.nmask;
    const bool up = w.r > 0, dn = w.r < H - 1, lf = w.c > 0, rt = w.c < W - 1;
    float cn = 0.f;
    if constexpr (kFirst) {
        if (a.route_cost) cn = cost[n];
    }
    float u[8];
    bool g[8];
    float umin = INF;
    fld_each<8>([&](auto k) __attribute__((always_inline)) {
        constexpr int A = decltype(k)::value;
        constexpr Move mv = kActionMoves[A];
        float x = INF;
        bool gg = false;
        if ((nm & fld_bit(mv.dy, mv.dx)) && fld_inside(mv.dy, mv.dx, up, dn, lf, rt)) {
            x = value(n + mv.dy * W + mv.dx, gg);
            if (!(fabsf(x) < INF)) x = INF;  // a candidate has a finite value
        }
        u[A] = x;
        g[A] = gg;
        umin = fminf(umin, x);
    });
    if (!(umin < INF)) {
        w.active = false;  // (a tape that is not these maps': the walk ends where it stands)
        return;
    }
    float uu;
    if (a.uniforms)
        uu = a.uniforms[row * (size_t)a.K + (size_t)j];
    else
        uu = (float)(srt_philox((uint32_t)j, (uint32_t)i, (uint32_t)q, 0u, a.key0, a.key1) >> 8) * 0x1p-24f;
    float wgt[8];
    float Z = 0.f;
    fld_each<8>([&](auto k) __attribute__((always_inline)) {
        constexpr int A = decltype(k)::value;
        wgt[A] = sfl_exp2(umin - u[A]);  // exp2(-inf) = 0: no candidate, and x + 0 is x
        Z += wgt[A];
    });
    const float t = uu * Z;
    float acc = 0.f;
    int ch = -1, last = -1;
    fld_each<8>([&](auto k) __attribute__((always_inline)) {
        constexpr int A = decltype(k)::value;
        if (u[A] < INF) {
            acc += wgt[A];
            last = A;
            if (ch < 0 && acc > t) ch = A;
        }
    });
    if (ch < 0) ch = last;  // rounding, u >= 1, a NaN u
    float uc = INF;
    bool gc = false;
    int step = 0, dy = 0, dx = 0;
    fld_each<8>([&](auto k) __attribute__((always_inline)) {
        constexpr int A = decltype(k)::value;
        constexpr Move mv = kActionMoves[A];
        if (ch == A) {
            uc = u[A];
            gc = g[A];
            dy = mv.dy;
            dx = mv.dx;
            step = mv.dy * W + mv.dx;
        }
    });
    if constexpr (kFirst) {
        if (a.visits) atomicAdd(&a.visits[q * ((size_t)H * W) + (size_t)n], 1);
        w.csum += (double)cn;
        if (a.log_prob) w.lsum += (double)(umin - uc) * M_LN2 - log((double)Z);
    }
    w.r += dy;
    w.c += dx;
    w.n += step;
    visit(w.n, w.len);
    ++w.len;
    if (gc) w.active = false;
}

// its launch for B * SN rows of `cap` cells and B * S planes of HW counts (a NULL is left alone; nothing is launched for two NULLs) -> a
// status.  Defined in nastar_soft_routes_capi.hip, the one translation unit that instantiates the kernel.
int soft_routes_clear(int32_t* routes, int32_t* visits, int B, int S, long long SN, int HW, int cap, hipStream_t s);

// blockIdx.x = map * groups + (slice of the map's S*N walkers); lane tid walks walker slice * T + tid.  R: the cells of a plane a lane
// stages per move (R * T >= H*W; the LDS kernel only)
template <int T, int R, bool LDS>
__global__ __launch_bounds__(T) void nastar_soft_routes_kernel(const SoftRoutesArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char srt_smem[];
    const int H = a.H, W = a.W, HW = H * W, K = a.K, tid = threadIdx.x;
    const float INF = INFINITY;
    float* buf = reinterpret_cast<float*>(srt_smem);
    const size_t stride = srt_plane_stride(HW);
    uint8_t* gb = reinterpret_cast<uint8_t*>(srt_smem + (LDS ? 2 * sfl_pad16((size_t)HW * 4) : 0));  // bit 0: goal, bit 1: passable goal
    int* flags = reinterpret_cast<int*>(srt_smem + soft_routes_lds_bytes(HW, LDS) - 32);
    const size_t map = blockIdx.x / (unsigned)a.groups;
    const int slice = (int)(blockIdx.x % (unsigned)a.groups);
    const float* cost = a.cost + map * (size_t)HW;
    const float* goal = a.goal + map * (size_t)HW;
    const float* pass = a.passable + map * (size_t)HW;
    const float* tape = a.tape + map * (size_t)K * HW;

    // ---- the map: the forward's BAD_COST rule, and the goal bytes ---------------------------------------------------------------------------
    if (tid < 8) flags[tid] = 0;
    __syncthreads();
    bool bad = false;
    for (int i = tid; i < HW; i += T) {
        const bool ok = pass[i] != 0.f;
        bad |= ok && !(cost[i] >= 0.f);  // NaN or negative on a passable cell (-0.0 >= 0)
        if constexpr (LDS) {
            const bool g = goal[i] != 0.f;
            gb[i] = (uint8_t)((g ? 1 : 0) | (g && ok ? 2 : 0));
        }
    }
    if (__ballot(bad) && (tid & 63) == 0) __hip_atomic_store(&flags[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    const bool map_bad = flags[1] != 0;

    // ---- the walker of this lane ------------------------------------------------------------------------------------------------------------
    const long long SN = (long long)a.S * a.N;
    const long long w = (long long)slice * T + tid;
    const bool has = w < SN;
    const int s = has ? (int)(w / a.N) : 0;
    const int i = has ? (int)(w - (long long)s * a.N) : 0;
    const size_t q = map * (size_t)a.S + (size_t)s;
    const size_t row = q * (size_t)a.N + (size_t)i;
    const int n0 = has ? a.start[q] : -1;
    const bool inside = n0 >= 0 && n0 < HW;
    const bool goal0 = inside && goal[n0] != 0.f;
    const float uK = inside ? tape[(size_t)(K - 1) * HW + n0] : INF;
    const int st = !inside ? NASTAR_ERR_BAD_SHAPE
                 : map_bad ? NASTAR_ERR_BAD_COST
                 : (!goal0 && !(fabsf(uK) < INF)) ? NASTAR_ERR_UNSOLVABLE
                                                  : NASTAR_OK;
    const bool ok = has && st == NASTAR_OK;

    // the value of plane p at cell i as the LDS kernel stages it: the tape's, or the implicit plane 0
    auto plane_cell = [&](int p, int cell) -> float {
        return p >= 1 ? tape[(size_t)(p - 1) * HW + cell] : (gb[cell] & 2) ? 0.f : INF;
    };

    // THE WALK.  first: the pass that tallies costs, log-probabilities and visits and writes the per-walker outputs; visit(cell, j) sees
    // route cell j.  -> the number of route cells
    auto walk = [&](auto first, auto visit) __attribute__((always_inline)) -> int {
        constexpr bool kFirst = decltype(first)::value;
        SrtWalker w{n0, 0, 0, 0, ok && !goal0, 0.0, 0.0};
        if (ok) {
            w.len = 1;
            visit(n0, 0);
            w.r = n0 / W;
            w.c = n0 - w.r * W;
        }
        if constexpr (LDS) {  // plane K - 1 into buffer 0, and the three "still on its way" flags (flags[4..6]) start at zero
            for (int cell = tid; cell < HW; cell += T) buf[cell] = plane_cell(K - 1, cell);
            if (tid < 3) flags[4 + tid] = 0;
            __syncthreads();
        }
        for (int j = 0; j < K; ++j) {  // the bound: no input moves it
            const int p = K - j - 1;   // the plane this move reads
            float stage[R];
            if constexpr (LDS) {
                if (p >= 1) {
#pragma unroll
                    for (int e = 0; e < R; ++e) {
                        const int cell = tid + e * T;
                        if (cell < HW) stage[e] = plane_cell(p - 1, cell);
                    }
                }
            }
            if (w.active) {
                const float* cur = LDS ? buf + (size_t)(j & 1) * stride : (p >= 1 ? tape + (size_t)(p - 1) * HW : nullptr);
                srt_move<kFirst>(a, cost, w, j, i, q, row, [&](int m, bool& gg) __attribute__((always_inline)) -> float {
                    if constexpr (LDS) {
                        gg = (gb[m] & 1) != 0;
                        return cur[m];
                    } else {
                        gg = goal[m] != 0.f;
                        return cur ? cur[m] : (gg && pass[m] != 0.f) ? 0.f : INF;
                    }
                }, visit);
            }
            if constexpr (LDS) {
                if (p >= 1) {
                    float* nxt = buf + (size_t)((j + 1) & 1) * stride;
#pragma unroll
                    for (int e = 0; e < R; ++e) {
                        const int cell = tid + e * T;
                        if (cell < HW) nxt[cell] = stage[e];
                    }
                }
                // "a walker is still on its way": one ballot per wavefront, a flag, ONE barrier per move -- three flags in rotation, as in
                // fld_sweep: the flag of move j is cleared during move j + 2, when nobody reads it.  (Not __syncthreads_or: it keeps a
                // static __shared__ word in front of the dynamic region.)
                const int slot = 4 + j % 3;
                if (__ballot(w.active) && (tid & 63) == 0) __hip_atomic_store(&flags[slot], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (tid == 0) __hip_atomic_store(&flags[slot == 6 ? 4 : slot + 1], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __syncthreads();
                if (__hip_atomic_load(&flags[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0) break;  // every walker has ended
            } else {
                if (!w.active) break;
            }
        }
        if constexpr (kFirst) {
            if (has) {
                a.len[row] = w.len;
                if (a.route_cost) a.route_cost[row] = ok ? (float)w.csum : INF;
                if (a.log_prob) a.log_prob[row] = ok ? (float)w.lsum : -INF;
                if (i == 0) a.status[q] = st;
            }
        }
        return w.len;
    };

    int32_t* out = a.routes ? a.routes + row * (size_t)a.cap : nullptr;  // (read by a lane with a walker only)
    if (!a.routes) {
        walk(std::true_type{}, [](int, int) {});
    } else if (a.cap >= K + 1) {  // no route outgrows the row: store on the way
        walk(std::true_type{}, [&](int cell, int j) { out[j] = cell; });
    } else {
        const int len = walk(std::true_type{}, [](int, int) {});
        const int skip = len - (len < a.cap ? len : a.cap);
        walk(std::false_type{}, [&](int cell, int j) {
            if (j >= skip) out[j - skip] = cell;
        });
    }
}

}  // namespace nastar
