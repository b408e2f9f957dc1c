// nastar_verdict.hip.h -- the proof that a batch is solvable (include/nastar_verdict.h): is every map's goal reachable from its start?
//
// The same bit-parallel wave as nastar_bfs_level_kernel (nastar_placement.hip.h: lane r holds row r of the map as a bit mask, one level =
// shifts + one DPP move up and down), but built to run BESIDE a search launch that fills the LDS of every CU and half its wave slots:
//   no LDS at all   the row masks are assembled in registers: the W / 4 lanes of a group load one 128- or 256-byte row as float4 -- every
//                   load instruction reads whole cache lines --, each lane shifts its bits into a word of its own, and one nibble transpose
//                   across the group (DPP butterfly) hands every lane its row
//   few wavefronts  a grid of at most one wavefront per SIMD; each loops over its share of the maps (launch shape: see kProofWavesPerSimd)
//   32x32           two maps per wavefront (lanes 0-31 and 32-63; the rows at a map's edge take nothing across it)
//   64x64           one map per wavefront, 64-bit masks
// Only reachability is wanted, not the level: the goal and a stalled wave are tested every 8 levels.
//
// Where the instruction slots go.  The wavefront is the youngest on a SIMD that holds four searching ones and issues in the slots they leave,
// so its duration follows the number of instructions it issues (and what it issues, it takes from the searches).  Counted in the gfx950
// listing of the 32x32 kernel, one tensor as cost and passable map, per pair of maps:
//   assembling the masks   about 480 slots (340 VALU: two per element for the bit, half a one for the cost range; 24 loads in one batch; no
//                          branch between the first load and the last transpose).  It was about 1100 executed of 1600 when every round
//                          OR-reduced its nibbles over the group and selected the owner's: 60 % of what a pair cost, not the flood
//   the flood              95 slots per 8 levels (7 VALU a level and the exit test); the bench's mazes need 53 levels on average for the
//                          longer map of a pair (start-goal distance: median 40, p90 61, maximum 107)
//   memory                 the loads of a pair are issued before the flood of the pair before it: one exposed round trip per wavefront
//                          where there were three per pair
// Measured beside the 4096-map search launch (profiles/lean_proof.json): 42 us where it took 83 (median), over 48 us into the search launch
// instead of 88; the search launch itself 118.2 us against 119.2 / 119.8.
#pragma once
#include "nastar_device.hip.h"

namespace nastar {

// Launch shape, measured beside the 4096-map 32x32 search launch ONLY, with the kernel of twice today's instruction count
// (profiles/early_verdict.json; not measured again since): one wavefront per SIMD -- two lengthen
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

// ---- assembling the row masks ------------------------------------------------------------------------------------------------------------
// Lane L of the wavefront owns row L & (W - 1) of map first_map + (L >> LOGW).  The G = W / 4 lanes of a group read one row per ROUND as
// float4, 16 bytes each (whole cache lines): in round k the row of the group's k-th lane.  A lane shifts the four bits of a round into ONE
// word of its own -- a compare and a carry-in add per element, no cross-lane step and no branch inside the rounds -- and after a BATCH of 8
// rounds holds an 8 x 4-bit column of the group's 8 x G nibble matrix.  One nibble transpose across the group (a butterfly: 3 stages inside a
// word, a fourth between the two words of a 64x64 row) then hands every lane its own row.
constexpr int kProofBatch = 8;  // rounds per batch: one 32-bit word per lane, 8 float4 = 32 VGPRs in flight

// the loads of one batch.  `maps`: the tensor at the group's first map (uniform); lane_off: this lane's byte offset from there (round 0);
// the rounds are immediate offsets
template <int LOGW>
__device__ __forceinline__ void proof_issue(float4 (&v)[kProofBatch], const float* __restrict__ maps, uint32_t lane_off, int part)
{
    constexpr int G = (1 << LOGW) / 4;
    const char* const p = reinterpret_cast<const char*>(maps) + lane_off;
#pragma unroll
    for (int k = 0; k < kProofBatch; ++k) v[k] = *reinterpret_cast<const float4*>(p + (part * kProofBatch + k) * G * 16);
}

// Bound (b) without a compare per element: as integers, the values 0 <= c <= c_max are the bit patterns 0 .. bits(c_max), -0.0 is
// 0x80000000, and everything else -- negative values, infinities, NaNs of either sign -- is a signed integer above bits(c_max) or an unsigned
// integer above 0x80000000.  So a signed and an unsigned running maximum decide a whole map: half an instruction per element each (max3).
struct ProofCostRange {
    int32_t smax = 0;
    uint32_t umax = 0;
    __device__ __forceinline__ void take(const float4& v)
    {
        const uint32_t x = __float_as_uint(v.x), y = __float_as_uint(v.y), z = __float_as_uint(v.z), w = __float_as_uint(v.w);
        smax = max(max(smax, (int32_t)x), (int32_t)y);
        smax = max(max(smax, (int32_t)z), (int32_t)w);
        umax = max(max(umax, x), y);
        umax = max(max(umax, z), w);
    }
    template <int LOGW>
    __device__ __forceinline__ bool bad() const { return smax > (int32_t)__float_as_uint(kProofMaxCost<LOGW>) || umax > 0x80000000u; }
};

// acc = 2 acc + (v != 0), NaN counting as non-zero: the compare's result is the carry into acc + acc.  (Written out: from C++ the compiler
// makes a select, a shift and an OR of it, and wait states between the compare and the select.)
__device__ __forceinline__ void proof_shift_in(uint32_t& acc, float v)
{
    asm("v_cmp_neq_f32_e32 vcc, 0, %1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc" : "+v"(acc) : "v"(v) : "vcc");
}

// one batch -> one word: bit 4 k + e = element e of round k is non-zero (shifted in from the top, reversed once at the end)
__device__ __forceinline__ uint32_t proof_word(const float4 (&v)[kProofBatch], bool bits, bool check, ProofCostRange& range)
{
    uint32_t acc = 0;
#pragma unroll
    for (int k = 0; k < kProofBatch; ++k) {
        if (bits) {
            proof_shift_in(acc, v[k].x);
            proof_shift_in(acc, v[k].y);
            proof_shift_in(acc, v[k].z);
            proof_shift_in(acc, v[k].w);
        }
        if (check) range.take(v[k]);
    }
    return __brev(acc);
}

// lane i of a group receives the value of lane i ^ D
template <int D>
__device__ __forceinline__ uint32_t proof_from_xor_lane(uint32_t v)
{
    if constexpr (D == 1) return dpp_mov<DPP_QUAD_XOR1>(v);
    else if constexpr (D == 2) return dpp_mov<DPP_QUAD_XOR2>(v);
    else if constexpr (D == 4) return dpp_mov<0x1B>(dpp_mov<DPP_ROW_HALF_MIRROR>(v));  // i ^ 7, then quad_perm:[3,2,1,0] = i ^ 3
    else return dpp_mov<0x128>(v);                                                    // row_ror:8 = i ^ 8 in a row of 16
}

// one butterfly stage of the nibble transpose inside a word: nibble j of lane i <-> nibble j ^ D of lane i ^ D wherever bit D of i and j differ
template <int D>
__device__ __forceinline__ uint32_t proof_transpose_stage(uint32_t own, int sub)
{
    constexpr uint32_t even = D == 1 ? 0x0F0F0F0Fu : D == 2 ? 0x00FF00FFu : 0x0000FFFFu;  // the nibbles whose index has bit D clear
    constexpr int LOGD = D == 1 ? 0 : D == 2 ? 1 : 2;
    const uint32_t upper = (uint32_t)-(int32_t)((sub >> LOGD) & 1);  // all ones in the lanes whose index has bit D set
    const uint32_t keep = even ^ upper;
    // a lane of the lower half takes their nibbles moved UP by D places, a lane of the upper half moved DOWN: a rotation serves both, the
    // bits that wrap fall outside ~keep
    const uint32_t theirs = __builtin_rotateleft32(proof_from_xor_lane<D>(own), (upper & (32 - 8 * D)) | (4 * D));
    return (own & keep) | (theirs & ~keep);
}

// the words a lane gathered (nibble k = its four columns of the group's k-th row) -> the mask of its own row
template <int LOGW>
__device__ __forceinline__ typename ProofRow<LOGW>::type proof_transpose(const uint32_t (&w)[(1 << LOGW) / 32], int sub)
{
    uint32_t t[(1 << LOGW) / 32];
#pragma unroll
    for (int i = 0; i < (1 << LOGW) / 32; ++i) t[i] = proof_transpose_stage<4>(proof_transpose_stage<2>(proof_transpose_stage<1>(w[i], sub), sub), sub);
    if constexpr (LOGW == 5) {
        return t[0];
    } else {
        const uint32_t lo = proof_from_xor_lane<8>(t[0]), hi = proof_from_xor_lane<8>(t[1]);
        return (sub & 8) ? ((uint64_t)hi | ((uint64_t)t[1] << 32)) : ((uint64_t)t[0] | ((uint64_t)lo << 32));
    }
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
// nastar_placement.hip.h (whose kernels live in another translation unit).  Written so that the move is the DPP operand of the AND
// (v_and_b32_dpp): the map-boundary rows are not a select per level, they are zero rows in the two copies of `pass` the AND takes
__device__ __forceinline__ uint32_t proof_and_from_below(uint32_t v, uint32_t m) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xF, 0xF, true) & m; }
__device__ __forceinline__ uint32_t proof_and_from_above(uint32_t v, uint32_t m) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xF, 0xF, true) & m; }
__device__ __forceinline__ uint64_t proof_and_from_below(uint64_t v, uint64_t m)
{
    return (uint64_t)proof_and_from_below((uint32_t)v, (uint32_t)m) | ((uint64_t)proof_and_from_below((uint32_t)(v >> 32), (uint32_t)(m >> 32)) << 32);
}
__device__ __forceinline__ uint64_t proof_and_from_above(uint64_t v, uint64_t m)
{
    return (uint64_t)proof_and_from_above((uint32_t)v, (uint32_t)m) | ((uint64_t)proof_and_from_above((uint32_t)(v >> 32), (uint32_t)(m >> 32)) << 32);
}

// Every group (MPW maps) of this wavefront's share; returns whether all of them were proved.  kSame: VanillaAstar hands ONE tensor over as
// cost map and obstacle map -- it is read once, and its range is tested on the values the mask is made of.
//
// The loads run as a stream of batches -- passable, start, goal (, cost), G / 8 batches each -- through a ring of kRing buffers: a buffer is
// loaded again as soon as its batch has been consumed, and the first kRing batches of the NEXT group are issued before this group's flood
// starts, so the flood (about a dozen live VGPRs) hides their round trip.  At 32x32 that is all of a group's passable, start and goal
// tensors: one exposed round trip per wavefront, none per group.
template <int LOGW, bool kSame>
__device__ __forceinline__ bool proof_groups(const float* __restrict__ cost, const float* __restrict__ start, const float* __restrict__ goal,
                                             const float* __restrict__ passable, int B, int* __restrict__ proved_out)
{
    using M = typename ProofRow<LOGW>::type;
    constexpr int W = 1 << LOGW, HW = W * W, MPW = 64 / W, G = W / 4, NW = W / 32;  // maps per wavefront, lanes per group, words per row
    constexpr int kTensors = kSame ? 3 : 4, kBatches = kTensors * NW, kRing = 3;
    const float* const tensor[4] = {passable, start, goal, cost};
    const int lane = threadIdx.x, r = lane & (W - 1), sub = lane & (G - 1);
    const int ngroups = (B + MPW - 1) / MPW;
    // what the previous trip assembled and this trip floods: the masks, the map, and whether (a), (b) hold.  Nothing in the first trip
    M pass = 0, pass_below = 0, pass_above = 0, vis = 0, gbit = 0;
    bool valid = false, sound = false;
    bool all_proved = true;
    for (int grp = blockIdx.x;; grp += gridDim.x) {
        const bool more = grp < ngroups;
        // After its last group a wavefront takes one more trip for that group's flood.  The loads are issued all the same -- straight-line
        // code: the compiler keeps loaded values that meet at a join in copies, and waits for the loads to make them -- but every lane then
        // reads the first 16 bytes of each row of a map it has just read: one request per instruction, nothing new from HBM
        const int first = (more ? grp : grp - (int)gridDim.x) * MPW;
        // (what a trip needs of the lane's number is worked out in the trip: carried across the flood it would hold VGPRs that the loads
        // in flight need -- the kernel sits at its 128)
        int l = lane;
        asm volatile("" : "+v"(l));
        const bool valid_next = more && first + (l >> LOGW) < B;
        // round 0 of this lane, in bytes from the group's first map.  A lane without a map reads the group's first map (which exists) and
        // drops what it read: no branch around the loads
        const int base = l & ~(G - 1);
        const uint32_t off = more ? (uint32_t)(((base & (W - 1)) * G + (l & (G - 1))) * 16 + (valid_next ? (base >> LOGW) * HW * 4 : 0)) : 0u;
        float4 buf[kRing][kProofBatch];
#pragma unroll
        for (int q = 0; q < kRing; ++q) proof_issue<LOGW>(buf[q], tensor[q / NW] + (size_t)first * HW, off, q % NW);
        __builtin_amdgcn_sched_barrier(0);
        // the flood: at least one new cell per level until it stalls, so HW / 8 rounds of 8 levels always suffice (empty masks stall at once)
        for (int round = 0; round <= HW / 8; ++round) {
            M prev = vis;
#pragma unroll
            for (int lvl = 0; lvl < 8; ++lvl) {
                prev = vis;
                // 7 VALU a level: two shifts, OR3; AND-OR (in the wait states a DPP read of h needs); the two ANDs that take their DPP move
                // as an operand; OR3.  (Left alone, the compiler regroups the ORs, keeps one move apart and needs 9: the empty statements
                // fix the grouping, nothing more)
                M h = vis | (vis << 1) | (vis >> 1);
                asm("" : "+v"(h));
                M same_row = (h & pass) | vis;
                asm("" : "+v"(same_row));
                M up = proof_and_from_below(h, pass_below), dn = proof_and_from_above(h, pass_above);
                asm("" : "+v"(up), "+v"(dn));
                vis = up | dn | same_row;
            }
            const uint64_t hit = __ballot((vis & gbit) != 0), moved = __ballot(vis != prev);
            bool over;  // every map of the wavefront has reached its goal or stalled (a map that is over floods on harmlessly)
            if constexpr (LOGW == 5) {
                const uint32_t hit0 = (uint32_t)hit, hit1 = (uint32_t)(hit >> 32), moved0 = (uint32_t)moved, moved1 = (uint32_t)(moved >> 32);
                over = ((hit0 != 0u) | (moved0 == 0u)) & ((hit1 != 0u) | (moved1 == 0u));
            } else {
                over = hit != 0ull || moved == 0ull;
            }
            if (over) break;
        }
        const bool reached = proof_own<LOGW>(__ballot((vis & gbit) != 0), lane) != 0ull;
        const bool proved = valid && sound && reached;
        if (proved_out != nullptr && valid && r == 0) proved_out[(grp - (int)gridDim.x) * MPW + (lane >> LOGW)] = proved ? 1 : 0;
        all_proved = all_proved && __ballot(valid && !proved) == 0ull;
        if (!more) break;
        // the next group's masks
        uint32_t w[3][NW];
        ProofCostRange range;
#pragma unroll
        for (int q = 0; q < kBatches; ++q) {
            const int t = q / NW;
            uint32_t word = proof_word(buf[q % kRing], t < 3, t == (kSame ? 0 : 3), range);
            // the batch is consumed HERE, before its buffer is loaded again (an empty statement the optimiser cannot move the arithmetic past)
            asm volatile("" : "+v"(word), "+v"(range.smax), "+v"(range.umax));
            if (t < 3) w[t][q % NW] = word;
            if (q + kRing < kBatches) {
                proof_issue<LOGW>(buf[q % kRing], tensor[(q + kRing) / NW] + (size_t)first * HW, off, (q + kRing) % NW);
                __builtin_amdgcn_sched_barrier(0);  // (the loads go out here, not where the scheduler would like them)
            }
        }
        pass = proof_transpose<LOGW>(w[0], sub), vis = proof_transpose<LOGW>(w[1], sub), gbit = proof_transpose<LOGW>(w[2], sub);
        valid = valid_next;
        if (!valid) pass = vis = gbit = 0;  // a lane without a map: empty masks, once (a group never straddles two maps, so the transpose mixes nothing)
        // rows 0 and W - 1 have no neighbour row in THEIR map (32x32: the wavefront's DPP shift would bring the other map's row in)
        pass_below = r == 0 ? (M)0 : pass, pass_above = r == W - 1 ? (M)0 : pass;
        const bool bad_cost = proof_own<LOGW>(__ballot(valid && range.bad<LOGW>()), lane) != 0ull;
        const bool has_start = proof_top_cell<LOGW>(vis, lane);
        const bool has_goal = proof_top_cell<LOGW>(gbit, lane);
        sound = !bad_cost && has_start && has_goal;
    }
    return all_proved;
}

// VGPRs: 127 (32x32) and 128 (64x64), up from 64 and 52.  The ring of batches in flight is 3 x 32 = 96 -- at 32x32 all of a pair's
// passable, start and goal maps --, the flood and the loop's own state take the rest.  Beside the launch this kernel is built for, a SIMD
// holds four searching wavefronts of 72 VGPRs and one of these: 4 x 72 + 128 <= 512, so 128 is free there (__launch_bounds__(64, 4)); more
// would not be.  NOT measured: launches whose searching wavefronts sit six to a SIMD (6 x 72 + 128 > 512), where a proof wavefront of
// 64 VGPRs found room and one of this size waits for a searching wavefront to end (at seven neither finds room).
template <int LOGW>
__global__ __launch_bounds__(64, 4) void nastar_solvable_proof_kernel(const float* __restrict__ cost, const float* __restrict__ start,
                                                                      const float* __restrict__ goal, const float* __restrict__ passable, int B,
                                                                      int* __restrict__ proved_out, int* word, int* counter)
{
    __builtin_amdgcn_s_setprio(kProofPriority);
    const int lane = threadIdx.x;
    const bool all_proved = passable == cost ? proof_groups<LOGW, true>(cost, start, goal, passable, B, proved_out)
                                             : proof_groups<LOGW, false>(cost, start, goal, passable, B, proved_out);
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
