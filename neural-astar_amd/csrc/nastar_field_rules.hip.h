// nastar_field_rules.hip.h -- the rules the four families of field kernels share, each written once: the
// move tables, the successor of a cell (fld_best_action), its children (fld_child_set), the in-place subtree sum of one cell
// (fld_subtree_sum) and the sweep-to-fixed-point loop (fld_sweep).  The tables are walked with compile-time indices (fld_each), so every
// mask test and every offset is a constant in the instruction stream.  No kernel lives here, so that several translation units may include it.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <utility>

namespace nastar {

constexpr int kFieldCellsPerLane = 16;  // 64 lanes x 16 = 1024 cells, 256 x 16 = 4096, 1024 x 16 = 16384

struct Move {
    int dy, dx;
};
constexpr Move kActionMoves[8] = {{-1, 0}, {0, 1}, {0, -1}, {1, 0}, {-1, 1}, {-1, -1}, {1, 1}, {1, -1}};   // synthetic.ACTION_MOVES
constexpr Move kChildOffsets[8] = {{-1, -1}, {-1, 0}, {-1, 1}, {0, -1}, {0, 1}, {1, -1}, {1, 0}, {1, 1}};  // row-major: the order of a sum
// the neighbour at kChildOffsets[j] steps onto this cell by the opposite move: action kOppositeAction[j]
constexpr int kOppositeAction[8] = {6, 3, 7, 1, 2, 4, 0, 5};
constexpr bool fld_opposites_hold()
{
    for (int j = 0; j < 8; ++j) {
        const Move m = kActionMoves[kOppositeAction[j]];
        if (m.dy != -kChildOffsets[j].dy || m.dx != -kChildOffsets[j].dx) return false;
    }
    return true;
}
static_assert(fld_opposites_hold(), "kOppositeAction[j] is the action whose move is minus kChildOffsets[j]");

// the mask bit of the move (dy, dx): filter cell (a, b) opens offset (1-a, 1-b) (include/nastar.h)
__device__ __forceinline__ constexpr uint32_t fld_bit(int dy, int dx) { return 1u << ((1 - dy) * 3 + (1 - dx)); }

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>), in that order
template <typename F, int... J>
__device__ __forceinline__ void fld_each_of(F&& f, std::integer_sequence<int, J...>)
{
    (f(std::integral_constant<int, J>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void fld_each(F&& f)
{
    fld_each_of(f, std::make_integer_sequence<int, N>{});
}

// table[k] for a k the lane knows at run time only: eight compares, no memory
template <const Move (&Table)[8]>
__device__ __forceinline__ Move fld_move(int k)
{
    Move r{0, 0};
    fld_each<8>([&](auto j) __attribute__((always_inline)) {
        constexpr Move m = Table[decltype(j)::value];
        if (k == decltype(j)::value) r = m;
    });
    return r;
}

// the move (dy, dx) stays inside the map, given the four border predicates of the cell
__device__ __forceinline__ bool fld_inside(int dy, int dx, bool up, bool dn, bool lf, bool rt)
{
    return (dy < 0 ? up : dy > 0 ? dn : true) && (dx < 0 ? lf : dx > 0 ? rt : true);
}

// THE POLICY: the first action, in ACTION_MOVES order, among the allowed in-map moves whose target has the smallest readable value
// at(dy, dx) -- a strict < keeps the first among equals -- taken only if that value is strictly below d; else -1
template <typename At>
__device__ __forceinline__ int fld_best_action(At at, uint32_t nm, bool up, bool dn, bool lf, bool rt, float d)
{
    float m = INFINITY;
    int best = -1;
    fld_each<8>([&](auto k) __attribute__((always_inline)) {
        constexpr Move mv = kActionMoves[decltype(k)::value];
        if ((nm & fld_bit(mv.dy, mv.dx)) && fld_inside(mv.dy, mv.dx, up, dn, lf, rt)) {
            const float v = at(mv.dy, mv.dx);
            if (v < m) {
                m = v;
                best = decltype(k)::value;
            }
        }
    });
    return m < d ? best : -1;
}

// THE CHILDREN of a cell: bit j = the neighbour at kChildOffsets[j] is inside the map and its successor byte succ_at(dy, dx) is the
// opposite move.  (A caller whose out-of-map neighbours read as "none" passes all-true predicates.)
template <typename SuccAt>
__device__ __forceinline__ uint32_t fld_child_set(SuccAt succ_at, bool up, bool dn, bool lf, bool rt)
{
    uint32_t kids = 0;
    fld_each<8>([&](auto j) __attribute__((always_inline)) {
        constexpr Move o = kChildOffsets[decltype(j)::value];
        if (fld_inside(o.dy, o.dx, up, dn, lf, rt) && succ_at(o.dy, o.dx) == kOppositeAction[decltype(j)::value]) kids |= 1u << decltype(j)::value;
    });
    return kids;
}

// the fp64 subtree sums in LDS: relaxed workgroup-scope 64-bit atomics -- ds_read_b64 / ds_write_b64, no data race in the language's sense
__device__ __forceinline__ double fgr_load(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void fgr_store(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// THE SUBTREE SUM of one cell, in place: A(v) = G(v) + A(c_0) + A(c_1) + ... in fp64, the children in kChildOffsets order, stored only
// when the BITS change (a NaN is a value like any other) -> changed.  A cell without a child is final from the start and is not touched.
__device__ __forceinline__ bool fld_subtree_sum(double* cell, int row_stride, uint32_t kids, float g)
{
    if (!kids) return false;
    double v = (double)g;
    fld_each<8>([&](auto j) __attribute__((always_inline)) {
        constexpr Move o = kChildOffsets[decltype(j)::value];
        if (kids & (1u << decltype(j)::value)) v += fgr_load(cell + o.dy * row_stride + o.dx);
    });
    if (__double_as_longlong(v) == __double_as_longlong(fgr_load(cell))) return false;
    fgr_store(cell, v);
    return true;
}

// THE SWEEP LOOP: body(backwards) visits every cell of the lane once, in place, and says whether it changed one; even sweeps run forwards,
// odd sweeps backwards (a lane's later visit reads what its earlier one wrote).  A sweep that changed nothing read final values only: the
// fixed point.  Detection: one ballot per wavefront, a flag in LDS, ONE barrier per sweep -- three flags in rotation (flags[0..2], zero on
// entry), so that the flag of sweep s is cleared during sweep s + 2, when nobody reads it.  `bound` is the caller's data-independent trip
// count.  -> the sweeps run, and whether the last one was quiet.  (The callables of this header are taken BY VALUE: a closure behind a
// reference kept the per-lane arrays it captures from being split into registers as well -- 6 VGPRs and an occupancy step in item 6g.)
struct Sweeps {
    int sweeps;
    bool quiet;
};
template <typename Body>
__device__ __forceinline__ Sweeps fld_sweep(int* flags, int bound, Body body)
{
    const int tid = threadIdx.x;
    for (int s = 0; s < bound; ++s) {  // the bound: no input moves it
        const bool changed = body((s & 1) != 0);
        const int slot = s % 3;
        if (__ballot(changed) && (tid & 63) == 0) __hip_atomic_store(&flags[slot], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (tid == 0) __hip_atomic_store(&flags[slot == 2 ? 0 : slot + 1], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __syncthreads();
        if (__hip_atomic_load(&flags[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0) return {s + 1, true};
    }
    return {bound, false};
}

}  // namespace nastar
