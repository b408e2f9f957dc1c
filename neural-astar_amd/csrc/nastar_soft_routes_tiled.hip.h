// nastar_soft_routes_tiled.hip.h -- the walkers of include/nastar_soft_routes_tiled.h: sampled routes from the maximum-entropy route
// distribution on maps above the one workgroup's, read from the tiled forward's checkpointed tape.
//
// The move of a walker is `srt_move` of nastar_soft_routes.hip.h, the statements the one-workgroup kernels run: the same bits.  What is new
// is that a walk is CUT: one launch serves one segment lo < k <= hi of the tape, whose planes lo .. hi - 1 the host has just rebuilt, and a
// walker lives in device memory between two launches (SoftRoutesTiledState: the cell, the length so far, "still on its way", the status
// of its query and the two fp64 sums -- the additions are the same sequence as in one launch).  The draw is a pure function of
// (seed, q, i, j), so the walk resumed is the walk.
//
// The shape is the gathering one of nastar_soft_routes.hip.h: 256 lanes, one walker per lane, eight dependent reads per move from the
// plane in device memory, no barrier, no LDS; the walkers of a map are split over workgroups and none waits for another.  A lane whose
// walker has ended returns before it reads anything else: a wavefront of ended walkers costs one load.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nastar_soft_routes_tiled.h"
#include "nastar_soft_routes.hip.h"

namespace nastar {

struct SoftRoutesTiledState {
    int32_t n, len;      // the cell the walker stands on; its route cells so far (0: a failed query)
    int32_t active, st;  // still on its way; the status of its query
    double csum, lsum;   // the fp64 tallies of route_cost and log_prob
};
static_assert(sizeof(SoftRoutesTiledState) == 32, "32 bytes per walker: what nastar_soft_routes_tiled_workspace_bytes counts");

enum { kSrtStoreNone = 0, kSrtStoreRows = 1, kSrtStoreTail = 2 };

struct SoftRoutesTiledArgs {
    SoftRoutesArgs a;             // (a.tape is not looked at: the planes are below)
    const float* plane_K;         // [B,HW]: the tape's last slot
    const float* first;           // [B,HW]: plane lo -- a checkpoint, or V_0 of the prepare launch
    const float* seg;             // planes lo + 1, lo + 2, ...: `plane` floats apart
    const int32_t* flags;         // [B,2] of the prepare launch: has_goal, bad_cost
    SoftRoutesTiledState* state;  // [B,S,N]
    size_t plane;                 // B * HW
    int lo, hi;                   // the moves of this launch: k = hi .. lo + 1 moves left
    int begin, end;               // the first launch of a pass forms the walkers, the last writes the per-walker outputs
    int store;                    // kSrtStoreNone; kSrtStoreRows: route cell l to row[l]; kSrtStoreTail: the last `cap` cells of a.len[row]
};

// blockIdx.x = map * groups + (slice of the map's S*N walkers); lane tid walks walker slice * T + tid.  kFirst: the pass that tallies and
// writes the per-walker outputs (the other pass is the replay of short rows: it stores cells and nothing else)
template <bool kFirst>
__global__ __launch_bounds__(kSoftRoutesGatherT) void nastar_soft_routes_tiled_kernel(const SoftRoutesTiledArgs t)
{
    constexpr int T = kSoftRoutesGatherT;
    const SoftRoutesArgs& a = t.a;
    const int W = a.W, HW = a.H * W, K = a.K;
    const float INF = INFINITY;
    const size_t map = blockIdx.x / (unsigned)a.groups;
    const int slice = (int)(blockIdx.x % (unsigned)a.groups);
    const long long SN = (long long)a.S * a.N;
    const long long wi = (long long)slice * T + (int)threadIdx.x;
    if (wi >= SN) return;
    const int s = (int)(wi / a.N);
    const int i = (int)(wi - (long long)s * a.N);
    const size_t q = map * (size_t)a.S + (size_t)s;
    const size_t row = q * (size_t)a.N + (size_t)i;
    const size_t base = map * (size_t)HW;
    const float* cost = a.cost + base;
    const float* goal = a.goal + base;
    SoftRoutesTiledState* sp = t.state + row;

    SrtWalker w{0, 0, 0, 0, false, 0.0, 0.0};
    int st = NASTAR_OK;
    if (!t.begin) {
        w.active = sp->active != 0;
        if (!w.active && !t.end) return;  // an ended walker: its state stays what it is
        w.n = sp->n;
        w.len = sp->len;
        st = sp->st;
        w.csum = sp->csum;
        w.lsum = sp->lsum;
    }

    int32_t* out = nullptr;
    int skip = 0;
    if (t.store != kSrtStoreNone) {
        out = a.routes + row * (size_t)a.cap;
        if (t.store == kSrtStoreTail) {  // (the replay: the first pass has written the length)
            const int len = a.len[row];
            skip = len - (len < a.cap ? len : a.cap);
        }
    }
    auto visit = [&](int cell, int l) __attribute__((always_inline)) {
        if (out && l >= skip) out[l - skip] = cell;
    };

    if (t.begin) {  // the status of the query, in the order of the header, and the walker on its start
        const int n0 = a.start[q];
        const bool inside = n0 >= 0 && n0 < HW;
        const bool goal0 = inside && goal[n0] != 0.f;
        const float uK = inside ? t.plane_K[base + (size_t)n0] : INF;
        const bool map_bad = t.flags[2 * map + 1] != 0;
        st = !inside ? NASTAR_ERR_BAD_SHAPE
           : map_bad ? NASTAR_ERR_BAD_COST
           : (!goal0 && !(fabsf(uK) < INF)) ? NASTAR_ERR_UNSOLVABLE
                                            : NASTAR_OK;
        const bool ok = st == NASTAR_OK;
        w.n = n0;
        w.active = ok && !goal0;
        if (ok) {
            w.len = 1;
            visit(n0, 0);
        }
    }
    if (w.active) {
        w.r = w.n / W;
        w.c = w.n - w.r * W;
    }

    for (int k = t.hi; w.active && k > t.lo; --k) {  // move j = K - k reads plane k - 1
        const int p = k - 1;
        const float* cur = (p == t.lo ? t.first : t.seg + (size_t)(p - t.lo - 1) * t.plane) + base;
        srt_move<kFirst>(a, cost, w, K - k, i, q, row, [&](int m, bool& gg) __attribute__((always_inline)) -> float {
            gg = goal[m] != 0.f;
            return cur[m];
        }, visit);
    }

    if (!t.end) {
        sp->n = w.n;
        sp->len = w.len;
        sp->active = w.active ? 1 : 0;
        sp->st = st;
        sp->csum = w.csum;
        sp->lsum = w.lsum;
        return;
    }
    if constexpr (kFirst) {
        const bool ok = st == NASTAR_OK;
        a.len[row] = w.len;
        if (a.route_cost) a.route_cost[row] = ok ? (float)w.csum : INF;
        if (a.log_prob) a.log_prob[row] = ok ? (float)w.lsum : -INF;
        if (i == 0) a.status[q] = st;
    }
}

}  // namespace nastar
