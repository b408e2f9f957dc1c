// nastar_soft_routes_grad.hip.h -- the score-function backward of the sampled routes: the weighted histogram of the routes the walkers
// wrote and the seed plane of the field's backward, both in fixed point (include/nastar_soft_routes_grad.h).
//
// Four kernels, in launch order; the field's backward (nastar_soft_fields_backward) runs between the third and the fourth:
//   scale      one workgroup per map: M_b = the largest |g| over the ok walkers as a bit pattern (the patterns of non-negative floats are
//              ordered as the numbers are; one at or above 0x7f800000 is an infinity or a NaN), kept as (e_b, kind); and the zeros of the
//              map's two int64 planes -- a launch, not a memset pair, as the clear in front of the walkers is.
//   histogram  a workgroup serves one map and a slice of its S*N walkers, ONE WAVEFRONT PER WALKER: the row is route_len contiguous int32,
//              read coalesced, 64 cells a round, and q is added per cell with a 64-bit integer LDS atomic into the workgroup's int64
//              plane of the map; the workgroup then adds its non-zero cells to the plane in device memory with 64-bit integer global
//              atomics.  Lane 0 adds q to Q_seed at the start cell, once per run of walkers of one query.  Integer sums: the order of the
//              adds and the split into workgroups cannot reach the bits.  No workgroup waits for another.  (The alternative, global
//              atomics straight from the rows with no LDS plane, gives the same bits and lost at every shape measured: DESIGN.md 6r.)
//   seed       seed = (float)(Q_seed * 2^(e_b - P)), every cell of every map.
//   combine    the store of the definition.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nastar_soft_routes_grad.h"
#include "nastar_soft_fields.hip.h"

namespace nastar {

constexpr int kSoftRoutesGradMaxCells = kSoftFieldsGradMaxCells;
constexpr int kSoftRoutesGradT = 256;        // the width of every workgroup here
constexpr int kSoftRoutesGradWalkers = 128;  // the walkers of one histogram workgroup: 32 per wavefront

enum { kSrgNormal = 0, kSrgZero = 1, kSrgNotFinite = 2 };  // the kind of a map's scale: M_b > 0 finite; 0 or no ok walker; an inf or a NaN

struct SrgScale {
    int32_t e;     // ilogb(M_b), kSrgNormal only
    int32_t kind;
};

struct SoftRoutesGradArgs {
    const int32_t* start;   // [B,S]
    const int32_t* routes;  // [B,S,N,cap]
    const int32_t* len;     // [B,S,N]
    const int32_t* status;  // [B,S]
    const float* g;         // [B,S,N]
    long long* q_visit;     // [B,HW]  (workspace)
    long long* q_seed;      // [B,HW]  (workspace)
    SrgScale* scale;        // [B]     (workspace)
    int groups;             // histogram workgroups per map
    int S, N, HW, K, cap;
    int P;
};

// LDS bytes of the histogram workgroup: the int64 plane of one map
constexpr size_t soft_routes_grad_lds_bytes(int HW) { return (size_t)HW * 8; }

// q of the definition: g in units of 2^(e - P), rounded to nearest, ties to even
__device__ __forceinline__ long long srg_quantise(float g, int e, int P) { return llrint(ldexp((double)g, P - e)); }

template <int T>
__global__ __launch_bounds__(T) void nastar_soft_routes_grad_scale_kernel(const SoftRoutesGradArgs a)
{
    __shared__ uint32_t top;
    const size_t map = blockIdx.x;
    const int tid = threadIdx.x;
    if (tid == 0) top = 0u;
    __syncthreads();
    const long long SN = (long long)a.S * a.N;
    uint32_t mine = 0u;
    bool any = false;
    for (long long w = tid; w < SN; w += T) {
        const size_t q = map * (size_t)a.S + (size_t)(w / a.N);
        if (a.status[q] == NASTAR_OK) {  // (the g of a walker that is not ok is not read)
            const uint32_t bits = __float_as_uint(a.g[map * (size_t)SN + (size_t)w]) & 0x7fffffffu;
            mine = bits > mine ? bits : mine;
            any = true;
        }
    }
    if (any) atomicMax(&top, mine);  // (an LDS integer atomic)
    long long* qv = a.q_visit + map * (size_t)a.HW;
    long long* qs = a.q_seed + map * (size_t)a.HW;
    for (int i = tid; i < a.HW; i += T) {
        qv[i] = 0;
        qs[i] = 0;
    }
    __syncthreads();
    if (tid == 0) {
        const uint32_t bits = top;
        SrgScale sc{0, kSrgZero};
        if (bits >= 0x7f800000u) {
            sc.kind = kSrgNotFinite;
        } else if (bits != 0u) {
            // (as a double every float is normal: the exponent field is ilogb, of a subnormal too)
            sc.e = (int32_t)((__double_as_longlong((double)__uint_as_float(bits)) >> 52) & 0x7ff) - 1023;
            sc.kind = kSrgNormal;
        }
        a.scale[map] = sc;
    }
}

// blockIdx.x = map * groups + (slice of the map's S*N walkers); wavefront v of the workgroup takes the slice's walkers v, v + T/64, ...
template <int T>
__global__ __launch_bounds__(T) void nastar_soft_routes_grad_histogram_kernel(const SoftRoutesGradArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char srg_smem[];
    const int HW = a.HW, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t map = blockIdx.x / (unsigned)a.groups;
    const int slice = (int)(blockIdx.x % (unsigned)a.groups);
    const SrgScale sc = a.scale[map];
    if (sc.kind != kSrgNormal) return;  // (uniform over the workgroup: the planes stay zero)
    unsigned long long* qv = reinterpret_cast<unsigned long long*>(a.q_visit) + map * (size_t)HW;
    unsigned long long* plane = reinterpret_cast<unsigned long long*>(srg_smem);
    for (int i = tid; i < HW; i += T) plane[i] = 0ull;
    __syncthreads();

    const long long SN = (long long)a.S * a.N;
    const long long first = (long long)slice * kSoftRoutesGradWalkers;
    const long long end = first + kSoftRoutesGradWalkers < SN ? first + kSoftRoutesGradWalkers : SN;
    unsigned long long* qs = reinterpret_cast<unsigned long long*>(a.q_seed) + map * (size_t)HW;
    long long seed_sum = 0;  // the q of the run of walkers of query seed_s this wavefront has met (lane 0 adds it where the run ends)
    long long seed_s = -1;
    auto flush_seed = [&]() {
        if (seed_s >= 0 && seed_sum != 0 && lane == 0) {
            const int n0 = a.start[map * (size_t)a.S + (size_t)seed_s];
            if ((unsigned)n0 < (unsigned)HW) atomicAdd(&qs[n0], (unsigned long long)seed_sum);
        }
    };
    for (long long w = first + wave; w < end; w += T / 64) {
        const long long s = w / a.N;
        if (a.status[map * (size_t)a.S + (size_t)s] != NASTAR_OK) continue;
        const size_t row = map * (size_t)SN + (size_t)w;
        const long long q = srg_quantise(a.g[row], sc.e, a.P);
        if (q == 0) continue;
        if (s != seed_s) {
            flush_seed();
            seed_s = s;
            seed_sum = 0;
        }
        seed_sum += q;
        int len = a.len[row];
        len = len < a.K + 1 ? len : a.K + 1;  // (cap >= K + 1: the row holds the whole route)
        const int32_t* cells = a.routes + row * (size_t)a.cap;
        for (int j = lane; j < len - 1; j += 64) {  // every route cell but the last
            const int n = cells[j];
            if ((unsigned)n < (unsigned)HW) atomicAdd(&plane[n], (unsigned long long)q);  // ds_add_u64; two's complement: the signed sum, exact
        }
    }
    flush_seed();
    __syncthreads();
    for (int i = tid; i < HW; i += T) {
        const unsigned long long v = plane[i];
        if (v != 0ull) atomicAdd(&qv[i], v);
    }
}

// seed[b,n] = (float)((double)Q_seed[b,n] * 2^(e_b - P)); zeros where the map's scale is not normal
template <int T>
__global__ __launch_bounds__(T) void nastar_soft_routes_grad_seed_kernel(const SoftRoutesGradArgs a, float* seed, size_t cells)
{
    const size_t stride = (size_t)gridDim.x * T;
    for (size_t i = (size_t)blockIdx.x * T + threadIdx.x; i < cells; i += stride) {
        const SrgScale sc = a.scale[i / (size_t)a.HW];
        seed[i] = sc.kind == kSrgNormal ? (float)ldexp((double)a.q_seed[i], sc.e - a.P) : 0.f;
    }
}

// grad_cost[b,n] = (float)(((double)A32[b,n] - (double)Q_visit[b,n] * 2^(e_b - P)) / tau); zeros on a BAD_COST map and where there was no
// weight, NaN where an ok walker's g was not finite
template <int T>
__global__ __launch_bounds__(T) void nastar_soft_routes_grad_combine_kernel(const SoftRoutesGradArgs a, const float* a32, const int32_t* map_status,
                                                                            double tau, float* grad_cost, size_t cells)
{
    const size_t stride = (size_t)gridDim.x * T;
    for (size_t i = (size_t)blockIdx.x * T + threadIdx.x; i < cells; i += stride) {
        const size_t map = i / (size_t)a.HW;
        const SrgScale sc = a.scale[map];
        float out = 0.f;
        if (map_status[map] == NASTAR_OK) {
            if (sc.kind == kSrgNotFinite)
                out = NAN;
            else if (sc.kind == kSrgNormal)
                out = (float)(((double)a32[i] - ldexp((double)a.q_visit[i], sc.e - a.P)) / tau);
        }
        grad_cost[i] = out;
    }
}

}  // namespace nastar
