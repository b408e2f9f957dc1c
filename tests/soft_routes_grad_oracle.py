"""The numpy restatement of include/nastar_soft_routes_grad.h: the score-function backward of the sampled routes.

log p(route) = (V_K(n_0) - cost(route)) / tau, so for an upstream gradient g of the walkers' log-probabilities

    grad_cost = (the field's backward of the plane that holds g summed at the start cells - the visits of the routes weighted with g) / tau

with both sums over walkers taken in FIXED POINT.  Everything below is written from the header: ``quantise`` (the scale of a map, P and the
integers q), ``q_planes`` (Q_visit and Q_seed, in Python integers: no width to overflow), ``seed_plane`` and ``combine`` (the two
conversions back, fp64 and one rounding).  ``expected`` puts them together around a callable for the field's backward -- on the device that
is ``ops.soft_fields_backward``, the existing kernel: the result is then defined to the bit.  ``reference`` is the same gradient in
float64 with no quantisation, from tests/soft_fields_oracle.py.
"""
import numpy as np

import soft_fields_oracle as SO

f32, f64 = np.float32, np.float64
NORMAL, ZERO, NOT_FINITE = 0, 1, 2   # the kind of a map's scale
MAX_BITS, MIN_BITS = 40, 30


def bits(S: int, N: int, K: int) -> int:
    """P = min(40, 61 - ceil(log2(S * N * K)))"""
    return min(MAX_BITS, 61 - (S * N * K - 1).bit_length())


def quantise(g, ok, S: int, N: int, K: int):
    """``g`` [B,S,N] float32, ``ok`` [B,S] bool -> (q [B,S,N] int64, 0 for a walker that is not ok; e [B] ints; P; kind [B]).  A map
    whose kind is not NORMAL has q = 0 and e = 0."""
    g = np.asarray(g, f32)
    B = g.shape[0]
    P = bits(S, N, K)
    assert P >= MIN_BITS, "a call the library refuses"
    q = np.zeros(g.shape, np.int64)
    e, kind = [0] * B, [ZERO] * B
    for b in range(B):
        mine = g[b][np.asarray(ok[b], bool)].astype(f64)          # (what is not ok is not read)
        if mine.size == 0:
            continue
        if not np.isfinite(mine).all():
            kind[b] = NOT_FINITE
            continue
        M = float(np.abs(mine).max())
        if M == 0.0:
            continue
        kind[b] = NORMAL
        e[b] = int(np.floor(np.log2(M)))                           # ilogb: exact in float64 for every float32, subnormal too
        while 2.0 ** e[b] > M:                                     # (guards the rounding of log2 next to a power of two)
            e[b] -= 1
        while 2.0 ** (e[b] + 1) <= M:
            e[b] += 1
        scaled = np.ldexp(g[b].astype(f64), P - e[b])              # exact: a shift of the exponent
        rows = np.asarray(ok[b], bool)
        q[b][rows] = np.rint(scaled[rows]).astype(np.int64)        # to nearest, ties to even: llrint
    return q, e, P, kind


def q_planes(routes, lengths, starts, q, HW: int):
    """one map: ``routes`` [S,N,cap] int, ``lengths`` [S,N], ``starts`` [S], ``q`` [S,N] (0 for a walker that is not ok) -> (Q_visit,
    Q_seed): lists of HW Python integers.  Every route cell but the last counts, a cell stood on twice counts twice."""
    S, N = np.asarray(q).shape
    qv, qs = [0] * HW, [0] * HW
    for s in range(S):
        for i in range(N):
            w = int(q[s][i])
            if w == 0:
                continue
            n0 = int(starts[s])
            if 0 <= n0 < HW:
                qs[n0] += w
            for n in np.asarray(routes[s][i][:max(0, int(lengths[s][i]) - 1)]).tolist():
                qv[n] += w
    return qv, qs


def _as_f64(ints):
    return np.array([float(v) for v in ints], f64)  # (int -> float64 rounds to nearest even, as the conversion of an int64 does)


def seed_plane(qs, e: int, P: int) -> np.ndarray:
    """[HW] float32: (float)((double)Q_seed * 2^(e - P))"""
    return (_as_f64(qs) * 2.0 ** (e - P)).astype(f32)


def combine(A32, qv, e: int, P: int, tau: float) -> np.ndarray:
    """[HW] float32: (float)(((double)A32 - (double)Q_visit * 2^(e - P)) / tau), rounded once"""
    return ((np.asarray(A32, f32).reshape(-1).astype(f64) - _as_f64(qv) * 2.0 ** (e - P)) / f64(tau)).astype(f32)


def expected(routes, lengths, starts, status, g, HW: int, K: int, tau: float, field_backward, map_status=None):
    """The whole definition for a batch -> grad_cost [B,HW] float32.  ``routes`` [B,S,N,cap], ``lengths`` [B,S,N], ``starts`` [B,S],
    ``status`` [B,S], ``g`` [B,S,N]; ``field_backward(seed [B,HW] float32) -> A32 [B,HW] float32`` is nastar_soft_fields_backward of the
    same maps; ``map_status`` [B]: a map with status 9 (BAD_COST) is all zeros."""
    B, S, N = np.asarray(g).shape
    ok = np.asarray(status) == 0
    q, e, P, kind = quantise(g, ok, S, N, K)
    planes = [q_planes(routes[b], lengths[b], starts[b], q[b], HW) for b in range(B)]
    seed = np.stack([seed_plane(planes[b][1], e[b], P) if kind[b] == NORMAL else np.zeros(HW, f32) for b in range(B)])
    A32 = np.asarray(field_backward(seed), f32).reshape(B, HW)
    out = np.zeros((B, HW), f32)
    for b in range(B):
        if map_status is not None and map_status[b] != 0:
            continue
        if kind[b] == NOT_FINITE:
            out[b] = np.nan
        elif kind[b] == NORMAL:
            out[b] = combine(A32[b], planes[b][0], e[b], P, tau)
    return out


def weighted_visits(routes, lengths, status, g, HW: int) -> np.ndarray:
    """one map, float64, no quantisation: [HW] the sum of g over the ok walkers and over every route cell but the last; and [HW] the
    unweighted counts"""
    S, N = np.asarray(g).shape
    w, cnt = np.zeros(HW, f64), np.zeros(HW, np.int64)
    for s in range(S):
        if status[s] != 0:
            continue
        for i in range(N):
            cells = np.asarray(routes[s][i][:max(0, int(lengths[s][i]) - 1)], np.int64)
            np.add.at(w, cells, f64(g[s][i]))
            np.add.at(cnt, cells, 1)
    return w, cnt


def seeds64(starts, status, g, HW: int) -> np.ndarray:
    """one map, float64: [HW] the sum of g over the ok walkers at their start cells"""
    out = np.zeros(HW, f64)
    for s in range(len(starts)):
        if status[s] == 0 and 0 <= int(starts[s]) < HW:
            out[int(starts[s])] += np.asarray(g[s], f64).sum()
    return out


def reference(cost, goal, passable, routes, lengths, starts, status, g, tau: float, K: int, mask):
    """one map ([H,W] arrays) in float64 with no quantisation -> (grad_cost [HW], the scale max|A_ref| + max|B_ref|) with A_ref = the
    field's backward / tau and B_ref = the weighted visits / tau, the two terms of the gradient: they can cancel, so an error is measured
    against their sizes, not against their difference"""
    H, W = np.asarray(cost).shape
    seed = seeds64(starts, status, g, H * W)
    A = SO.soft_field_grad(cost, goal, passable, seed.reshape(H, W), tau, K, mask).grad.reshape(-1)
    Bv, _ = weighted_visits(routes, lengths, status, g, H * W)
    return (A - Bv) / tau, float(np.abs(A).max() + np.abs(Bv).max()) / tau


# ---- the cases the CPU and the GPU tests share ---------------------------------------------------------------------------------------------------
# (H, W, B, seed) of soft_fields_oracle.SHAPE_CASES up to 1023 cells: a goal alone; one row, one column; fewer cells than a wavefront with
# B = 3 and an odd H*W; 256 cells; 257, one row longer than a wavefront reads in four rounds; 1023 cells
SHAPE_CASES = ((1, 1, 1, 1), (1, 9, 1, 2), (9, 1, 1, 3), (5, 7, 3, 4), (16, 16, 2, 7), (1, 257, 1, 8), (31, 33, 3, 5))


def cases(H, W, B, seed):
    """(K, tau, mask, (S, N), sample seed) of one shape: every (horizon, tau, mask) of soft_fields_oracle.sweep_cases, the walker counts
    of soft_routes_oracle.WALKERS -- 1, 15, 64, 65 and 300 walkers per map -- taken in turn so that each count meets each shape"""
    import soft_routes_oracle as RO
    _, passable, goal = RO.case_maps(H, W, B, seed)
    for k, (K, tau, mask) in enumerate(SO.sweep_cases(goal[0], passable[0])):
        yield K, tau, mask, RO.WALKERS[(k + seed) % len(RO.WALKERS)], 1000 * seed + k


# ---- the bound the GPU tests hold the kernels to ---------------------------------------------------------------------------------------------
# tests/test_soft_routes_grad_gpu.py compares the gradient with ``reference`` within soft_fields_oracle.BWD_RTOL of that scale: the
# committed bound of the ONE kernel that rounds in float32 here, the field's backward; the histogram adds 2^-39 of M_b per visit and the
# store one rounding.  Measured on the cases of that file (MI355X, the worst case -- the 31x33 maps -- printed by
# test_gradient_against_float64; a record, as soft_routes_oracle.LOGP_KERNELS is, not a bound):
GRAD_KERNELS = 6.55e-06
