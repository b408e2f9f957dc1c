// nastar_verdict.hip.h -- the proof that a batch is solvable (include/nastar_verdict.h): is every map's goal reachable from its start?
//
// The same bit-parallel wave as nastar_bfs_level_kernel (nastar_placement.hip.h: lane r holds row r of the map as a bit mask, one level =
// shifts + one DPP move up and down), but built to run BESIDE a search launch that fills the LDS of every CU and half its wave slots:
//   no LDS at all   the row masks are assembled in registers: the W / 4 lanes of a group load one 128- or 256-byte row as float4, OR their
//                   nibbles together by DPP, and the lane whose row it is keeps the result -- every load instruction reads whole cache lines
//   few wavefronts  a grid of at most one wavefront per SIMD; each loops over its share of the maps (launch shape: see kProofWavesPerSimd)
//   32x32           two maps per wavefront (lanes 0-31 and 32-63; the DPP move across the halves is masked off)
//   64x64           one map per wavefront, 64-bit masks
// Only reachability is wanted, not the level: the goal and a stalled wave are tested every 8 levels.
#pragma once
#include "nastar_device.hip.h"

namespace nastar {

// Launch shape, measured beside the 4096-map 32x32 search launch ONLY (profiles/early_verdict.json): one wavefront per SIMD -- two lengthen
// that search launch from 120 to 141 us -- at the search loop's own priority: at priority 0 the proof only issues when no searching
// wavefront of its SIMD can (it then ends 95 us into the search launch instead of 85 us, and the step gains half as much); the search
// launch's own duration is the same either way (120.0 / 120.6 us, 119.5 us without a proof beside it).  NOT measured: 64x64 batches, and
// launches whose search wavefronts sit eight to a SIMD (several batches in flight): there a proof at priority 3 competes with searches on
// equal terms, and priority 0 may be the better choice.
constexpr int kProofWavesPerSimd = 1;
constexpr int kProofPriority = 3;
// Bound (b) on the costs.  "A finished map is at a fixed point of the batch loop" is an inequality between two fp32 keys (the COUPLED test of
// nastar_forward_compact_body.inc): key(g + c_goal, omg (h0(n) + c_n)) > key(g, omg c_goal) for every neighbour n of the goal, omg = 1 - g_ratio.
// In exact arithmetic the two sides differ by (2 g_ratio - 1) c_goal + omg (h0(n) + c_n) >= omg, since h0(n) >= 1.  In fp32 every operand is
// at most M = H W c_max + c_max + 96 (a route has fewer than H W cells, h0 < 96 on a 64x64 map); the eight roundings of the two sums cost at
// most 8 u M and the two roundings of the division by sqrt(W) at most 2 u M more (u = 2^-24, every rounding monotone), so the keys stay
// strictly ordered while omg > 10 u M.  The proof keeps M <= 2^16, i.e. 10 u M <= 0.04: a factor of 6 below omg >= 0.25, which is g_ratio in
// [0.5, 0.75] -- the range in which the callers use it (ops.PROOF_MAX_G_RATIO).  Per cell: 60 on a 32x32 map, 15 on a 64x64 map.
constexpr float kProofMaxRouteCost = 61440.f;    // H W c_max; + c_max + 96 stays below 2^16
template <int LOGW>
constexpr float kProofMaxCost = kProofMaxRouteCost / (float)(1 << (2 * LOGW));
constexpr unsigned kProofFailBit = 0x40000000u;  // in the completion counter: some workgroup met a map it could not prove
constexpr unsigned kProofCountMask = 0x000FFFFFu;

template <int LOGW>
struct ProofRow {
    using type = uint32_t;
};
template <>
struct ProofRow<6> {
    using type = uint64_t;
};

// OR over the G (8 or 16) lanes of a group, result in every lane of the group
template <int G>
__device__ __forceinline__ uint32_t proof_group_or(uint32_t v)
{
    v |= dpp_mov<DPP_QUAD_XOR1>(v);
    v |= dpp_mov<DPP_QUAD_XOR2>(v);
    v |= dpp_mov<DPP_ROW_HALF_MIRROR>(v);
    if constexpr (G == 16) v |= dpp_mov<DPP_ROW_MIRROR>(v);
    return v;
}

__device__ __forceinline__ uint32_t proof_nibble(const float4& v)
{
    return (v.x != 0.f ? 1u : 0u) | (v.y != 0.f ? 2u : 0u) | (v.z != 0.f ? 4u : 0u) | (v.w != 0.f ? 8u : 0u);
}

template <int LOGW>
__device__ __forceinline__ bool proof_cost_ok(float c) { return c >= 0.f && c <= kProofMaxCost<LOGW>; }  // NaN fails both, -0.0 passes

// Row mask of THIS lane's row (bit c = cell c of the row is non-zero) of one tensor.  Lane L of the wavefront owns row L & (W - 1) of map
// first_map + (L >> LOGW).  In round k the G lanes of a group load the row of the group's k-th lane, 16 bytes each.  `valid`: the lane's map
// exists (a group never straddles two maps).  kCheck: `bad` collects cost values outside [0, kProofMaxCost<LOGW>] (per lane: four cells a round).
template <int LOGW, bool kCheck>
__device__ __forceinline__ typename ProofRow<LOGW>::type proof_row_mask(const float4* __restrict__ t4, int first_map, bool valid, int lane, bool& bad)
{
    using M = typename ProofRow<LOGW>::type;
    constexpr int W = 1 << LOGW, G = W / 4, Q = W * W / 4;
    const int sub = lane & (G - 1), base = lane & ~(G - 1);
    // a lane without a map reads the wavefront's first map (which exists) and drops what it read: no branch around the loads.  Round k is
    // k * G float4 further on: one address per lane, the rounds are immediate offsets
    const float4* const p = t4 + (size_t)first_map * Q + ((valid ? (base >> LOGW) : 0) * Q + (base & (W - 1)) * G + sub);
    M mine = 0;
    constexpr int NB = 8;  // loads in flight, 4 VGPRs each
#pragma unroll 1
    for (int k0 = 0; k0 < G; k0 += NB) {  // (32x32: one trip, 64x64: two)
        float4 v[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) v[k] = p[(k0 + k) * G];
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            if constexpr (kCheck) bad |= valid && !(proof_cost_ok<LOGW>(v[k].x) && proof_cost_ok<LOGW>(v[k].y) && proof_cost_ok<LOGW>(v[k].z) && proof_cost_ok<LOGW>(v[k].w));
            const uint32_t nib = valid ? proof_nibble(v[k]) : 0u;
            M m;
            if constexpr (LOGW == 5) {
                m = proof_group_or<G>(nib << (4 * sub));
            } else {
                // each half of the 16-lane group assembles one 32-bit word of the row; the mirror move fetches the other half's
                const uint32_t own = proof_group_or<8>(nib << (4 * (sub & 7))), other = dpp_mov<DPP_ROW_MIRROR>(own);
                m = sub < 8 ? ((uint64_t)own | ((uint64_t)other << 32)) : ((uint64_t)other | ((uint64_t)own << 32));
            }
            if (sub == k0 + k) mine = m;
        }
        __builtin_amdgcn_sched_barrier(0);  // (the next batch's loads stay behind this batch's masks: register pressure)
    }
    return mine;
}

// the bits of a ballot that belong to this lane's map
template <int LOGW>
__device__ __forceinline__ uint64_t proof_own(uint64_t ballot, int lane)
{
    if constexpr (LOGW == 5) return (lane & 32) ? (ballot >> 32) : (ballot & 0xFFFFFFFFull);
    return ballot;
}

// a one-hot map's cell by compact_load_map's rule -- the non-zero cell with the HIGHEST index: the highest row that holds one, its highest
// bit.  Returns whether the map holds a non-zero cell at all (uniform over the map's lanes); `mask` becomes that one bit (0 in every other row).
template <int LOGW>
__device__ __forceinline__ bool proof_top_cell(typename ProofRow<LOGW>::type& mask, int lane)
{
    using M = typename ProofRow<LOGW>::type;
    constexpr int W = 1 << LOGW;
    const uint64_t rows = proof_own<LOGW>(__ballot(mask != 0), lane);
    if (rows == 0ull) return false;
    const int top = 63 - __clzll((long long)rows);
    if ((lane & (W - 1)) != top) mask = 0;
    else if constexpr (LOGW == 5) mask = (M)1 << (31 - __clz((int)mask));
    else mask = (M)1 << (63 - __clzll((long long)mask));
    return true;
}

// lane i receives the value of lane i-1 / i+1 of the whole wavefront (0 at the ends): DPP wave_shr:1 / wave_shl:1, the idiom of
// nastar_placement.hip.h (whose kernels live in another translation unit)
__device__ __forceinline__ uint32_t proof_wave_from_below(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xF, 0xF, true); }
__device__ __forceinline__ uint32_t proof_wave_from_above(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xF, 0xF, true); }

template <int LOGW>
__device__ __forceinline__ typename ProofRow<LOGW>::type proof_from_below(typename ProofRow<LOGW>::type h)
{
    if constexpr (LOGW == 5) return proof_wave_from_below(h);
    else return (uint64_t)proof_wave_from_below((uint32_t)h) | ((uint64_t)proof_wave_from_below((uint32_t)(h >> 32)) << 32);
}
template <int LOGW>
__device__ __forceinline__ typename ProofRow<LOGW>::type proof_from_above(typename ProofRow<LOGW>::type h)
{
    if constexpr (LOGW == 5) return proof_wave_from_above(h);
    else return (uint64_t)proof_wave_from_above((uint32_t)h) | ((uint64_t)proof_wave_from_above((uint32_t)(h >> 32)) << 32);
}

// (64 threads, 8 wavefronts per SIMD: at most 64 VGPRs)
template <int LOGW>
__global__ __launch_bounds__(64, 8) void nastar_solvable_proof_kernel(const float* __restrict__ cost, const float* __restrict__ start,
                                                                      const float* __restrict__ goal, const float* __restrict__ passable, int B,
                                                                      int* __restrict__ proved_out, int* word, int* counter)
{
    using M = typename ProofRow<LOGW>::type;
    constexpr int W = 1 << LOGW, HW = W * W, MPW = 64 / W;  // maps per wavefront
    __builtin_amdgcn_s_setprio(kProofPriority);
    const int lane = threadIdx.x, r = lane & (W - 1);
    const bool same_cp = passable == cost;  // VanillaAstar hands ONE tensor over as cost map and obstacle map: read it once
    // rows 0 and W - 1 have no neighbour row in THEIR map (32x32: the wavefront's DPP shift would bring the other map's row in)
    const M keep_below = r == 0 ? (M)0 : ~(M)0, keep_above = r == W - 1 ? (M)0 : ~(M)0;
    const int ngroups = (B + MPW - 1) / MPW;
    bool all_proved = true;
    for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const int first = grp * MPW, b = first + (lane >> LOGW);
        const bool valid = b < B;
        bool bad = false, unused = false;
        M pass;
        if (same_cp) {
            pass = proof_row_mask<LOGW, true>(reinterpret_cast<const float4*>(cost), first, valid, lane, bad);
        } else {
            pass = proof_row_mask<LOGW, false>(reinterpret_cast<const float4*>(passable), first, valid, lane, unused);
            (void)proof_row_mask<LOGW, true>(reinterpret_cast<const float4*>(cost), first, valid, lane, bad);
        }
        M vis = proof_row_mask<LOGW, false>(reinterpret_cast<const float4*>(start), first, valid, lane, unused);
        M gbit = proof_row_mask<LOGW, false>(reinterpret_cast<const float4*>(goal), first, valid, lane, unused);
        const bool bad_cost = proof_own<LOGW>(__ballot(bad), lane) != 0ull;
        const bool has_start = proof_top_cell<LOGW>(vis, lane);
        const bool has_goal = proof_top_cell<LOGW>(gbit, lane);
        // the flood: at least one new cell per level until it stalls, so HW / 8 rounds of 8 levels always suffice
        for (int round = 0; round <= HW / 8; ++round) {
            M prev = vis;
#pragma unroll
            for (int lvl = 0; lvl < 8; ++lvl) {
                prev = vis;
                const M h = vis | (vis << 1) | (vis >> 1);
                const M up = proof_from_below<LOGW>(h) & keep_below, dn = proof_from_above<LOGW>(h) & keep_above;
                vis = ((h | up | dn) & pass) | vis;
            }
            const uint64_t hit = __ballot((vis & gbit) != 0), moved = __ballot(vis != prev);
            bool over;  // every map of the wavefront has reached its goal or stalled (a map that is over floods on harmlessly)
            if constexpr (LOGW == 5)
                over = ((uint32_t)hit != 0u || (uint32_t)moved == 0u) && ((uint32_t)(hit >> 32) != 0u || (uint32_t)(moved >> 32) == 0u);
            else
                over = hit != 0ull || moved == 0ull;
            if (over) break;
        }
        const bool reached = proof_own<LOGW>(__ballot((vis & gbit) != 0), lane) != 0ull;
        const bool proved = valid && !bad_cost && has_start && has_goal && reached;
        if (proved_out != nullptr && valid && r == 0) proved_out[b] = proved ? 1 : 0;
        all_proved = all_proved && __ballot(valid && !proved) == 0ull;
    }
    // the terminal word, by the pattern of the search's completion flag (nastar_search_kernels.hip.h: note_done): release, count, and the workgroup that
    // counts last publishes with a system-scope store.  The counter carries "some map was not proved" in a high bit and is 0 again first.
    if (lane == 0) {
        __threadfence();
        if (!all_proved) atomicOr(reinterpret_cast<unsigned*>(counter), kProofFailBit);  // (before this workgroup counts itself: the last count sees it)
        const unsigned old = atomicAdd(reinterpret_cast<unsigned*>(counter), 1u);
        if ((old & kProofCountMask) == gridDim.x - 1u) {
            const bool fail = (old & kProofFailBit) != 0u;
            __hip_atomic_store(counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __threadfence_system();
            __hip_atomic_store(word, fail ? 2 : 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

}  // namespace nastar
