"""Sampled routes from the maximum-entropy route distribution in numpy: the DEFINITION of include/nastar_soft_routes.h (DESIGN.md section 2,
item 6p) -- Philox4x32-10 and a float64 walker over given planes [V_0 .. V_K].

The walker (b, s, i) stands on n_0; at move j it has k = K - j moves left; on a goal the route ends; otherwise the candidates are the
allowed moves n -> m with V_{k-1}(m) finite, the weights exp(-(V_{k-1}(m) - min) / tau) over them in action order, Z their sequential sum,
t = u * Z, and the chosen action is the first whose running sum is > t, else the last candidate.  Everything here is float64: a float32
kernel that reads float32 planes draws the same action unless t falls within rounding of a boundary of the running sum -- such a draw is
FRAGILE, and ``walk`` reports per route whether it made one.

    fragile    |acc - t| <= band * (acc + t) at a boundary other than the last candidate's (behind the last there is nothing to cross)
    band       4 * 2^-24 * max|V| / tau + 64 * 2^-24.  The first term: a log-weight is a difference of two plane values, and the planes a
               test hands over are the kernel's V = U * tau * ln 2 rounded at their store, while the kernel reads U: two roundings of
               2^-24 |V| each per value, divided by tau.  The second: the exp2 of the device (1 ulp), eight additions, the product u * Z.
    floor      ... + 2^-120 on the right-hand side: a float32 weight below 2^-126 (2^-149 with denormals) is 0, so a float32 running sum
               cannot tell such a sum from 0 where float64 can.  It matters for u = 0 exactly (the crafted rows of the ``uniforms``
               tests) at a small tau, where the first candidates' weights underflow: float64 takes the first of them, float32 the first
               whose weight is not 0.

Measured (the shares of FRAGILE routes, and the routes that differ among the others -- which must be none):
    the issue that asked for this: float32 stand-ins for the device on 16x16 maps, K = 64, 1224 routes per tau:
               tau 1.0: 1.8 % flagged, 0 mismatches; tau 0.1: 0 %, 0; tau 0.02: 0.1 %, 0
    the cases below (``oracle_cases``: per (shape, horizon, tau, mask) the routes of every walker count, from Philox and from the crafted
    uniforms), float32 stand-in (``walk`` with dtype=float32 on the float32 planes of tests/soft_fields_oracle.py, this numpy) and kernels
    (MI355X, tests/test_soft_routes_gpu.py::test_routes_are_the_oracles) alike, flag for flag: no mismatch anywhere; the worst case is
    31x33, K = 128, tau = 1.0, Moore-8 with 52 of 1666 routes (3.1 %), then 31x33, K = 50, tau = 0.02, 4-connected with 2.6 %; every
    case up to 16x16 is below 1.5 %, the 96x128 case at 0.5 %.  ``FRAGILE_MEASURED``; the bound is the 5 % the issue set, not a
    measurement.  The sample seeds were re-checked on the stand-in before they were committed (the issue asks for it): with the first
    choice, 1000 * seed, the worst case stood at 4.97 % -- its routes take all 128 moves at max|V| / tau = 200, and a third of a case's
    routes start on a goal or not at all, so the share moves with the starts the seed draws.
"""
import os
import sys
from typing import NamedTuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fields_oracle import ACTION_MOVES  # noqa: E402
from heuristic_oracle import MOORE8, offsets  # noqa: E402

f32, f64, u32, u64 = np.float32, np.float64, np.uint32, np.uint64
STATUS_OK, STATUS_BAD_START, STATUS_UNSOLVABLE, STATUS_BAD_COST = 0, 1, 3, 9
FRAGILE_MAX_SHARE = 0.05
FLOOR = 2.0 ** -120  # see the module docstring

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
# (counter, key, output): the known answers of Philox4x32-10 (Random123's kat_vectors)
PHILOX_KNOWN = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def philox4x32_10(counter, key):
    """counter: four, key: two arrays (or ints) of 32-bit words, broadcast against each other -> the four output words, uint32 arrays"""
    c = [np.asarray(x, u64) & u64(0xffffffff) for x in counter]
    k = [np.asarray(x, u64) & u64(0xffffffff) for x in key]
    mask = u64(0xffffffff)
    for _ in range(10):
        p0, p1 = u64(PHILOX_M0) * c[0], u64(PHILOX_M1) * c[2]
        c = [(p1 >> u64(32)) ^ c[1] ^ k[0], p1 & mask, (p0 >> u64(32)) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + u64(PHILOX_W0)) & mask, (k[1] + u64(PHILOX_W1)) & mask]
    return [x.astype(u32) for x in c]


def uniform(seed: int, q, i, j) -> np.ndarray:
    """the u of walker (query q, sample i) at move j: (x0 >> 8) * 2^-24, float64 (exact)"""
    seed &= (1 << 64) - 1
    x0 = philox4x32_10((j, i, q, 0), (seed & 0xffffffff, seed >> 32))[0]
    return (x0 >> u32(8)).astype(f64) * 2.0 ** -24


def band(planes, tau: float) -> float:
    fin = [np.abs(np.asarray(V, f64)[np.isfinite(V)]) for V in planes]
    vmax = max((float(a.max()) for a in fin if a.size), default=0.0)
    return 4 * 2.0 ** -24 * vmax / tau + 64 * 2.0 ** -24


class Routes(NamedTuple):
    cells: list              # per walker: the route's flat cell indices in travel order ([] for a failed query)
    cost: np.ndarray         # [n] float64: the cost of every route cell but the last (+inf for a failed query)
    log_prob: np.ndarray     # [n] float64 (-inf for a failed query)
    fragile: np.ndarray      # [n] bool: the route made a fragile draw
    status: np.ndarray       # [n] int32: the status of the walker's query


def walk(planes, cost, goal, passable, starts, tau, mask, u_of, dtype=f64) -> Routes:
    """``planes`` [V_0 .. V_K] ([H,W] each, as the recursion reads them: +inf on every obstacle) or None for a BAD_COST map; ``starts`` [n]
    flat start cells, one per walker; ``u_of(j)`` -> [n] the walkers' u at move j.  All n walkers advance together, move by move.
    ``dtype=np.float32`` runs the draw's statements in float32 (the stand-in for a float32 kernel); the tallies stay float64."""
    dt = np.dtype(dtype).type
    cost, gl, ok = np.asarray(cost, f64), np.asarray(goal) != 0, np.asarray(passable) != 0
    H, W = cost.shape
    starts = np.asarray(starts, np.int64)
    n = starts.size
    inside = (starts >= 0) & (starts < H * W)
    s0 = np.where(inside, starts, 0)
    r, c = s0 // W, s0 % W
    status = np.full(n, STATUS_OK, np.int32)
    if planes is None:
        status[:] = STATUS_BAD_COST
    else:
        K = len(planes) - 1
        status[~gl[r, c] & ~np.isfinite(np.asarray(planes[K])[r, c])] = STATUS_UNSOLVABLE
        bnd = band(planes, tau)
    status[~inside] = STATUS_BAD_START
    good = status == STATUS_OK
    cells = [[int(s)] if g else [] for s, g in zip(s0, good)]
    csum = np.where(good, 0.0, np.inf)
    lsum = np.where(good, 0.0, -np.inf)
    fragile = np.zeros(n, bool)
    active = good & ~gl[r, c]
    moves = [mv for mv in ACTION_MOVES if mv in offsets(mask)]
    j = 0
    while active.any():
        assert j < K, "a walker outlived the horizon: the planes are not these maps'"
        V = np.pad(np.asarray(planes[K - j - 1]).astype(dtype), 1, constant_values=np.inf)
        w = np.flatnonzero(active)
        X = np.stack([V[r[w] + 1 + dy, c[w] + 1 + dx] for dy, dx in moves])          # [moves, walkers]
        cand = np.isfinite(X)
        assert cand.any(0).all(), "a live cell without a candidate"
        vmin = np.where(cand, X, np.inf).min(0)
        with np.errstate(invalid="ignore", under="ignore"):
            logw = np.where(cand, -(X - vmin) / dt(tau), -np.inf).astype(dtype)
            wgt = np.where(cand, np.exp(logw), dt(0)).astype(dtype)
        acc = np.cumsum(wgt, 0, dtype=dtype)                                            # the sequential sum, in action order
        Z = acc[-1]
        u = np.asarray(u_of(j), f64)[w].astype(dtype)
        t = (u * Z).astype(dtype)
        last = len(moves) - 1 - np.argmax(cand[::-1], 0)
        with np.errstate(invalid="ignore"):
            over = cand & (acc > t)
            chosen = np.where(over.any(0), np.argmax(over, 0), last)
            near = cand & (np.abs(acc - t) <= bnd * (acc + t) + FLOOR) & (np.arange(len(moves))[:, None] != last)
        fragile[w] |= near.any(0)
        csum[w] += cost[r[w], c[w]]
        lsum[w] += logw[chosen, np.arange(w.size)].astype(f64) - np.log(Z.astype(f64))
        dy = np.array([mv[0] for mv in moves])[chosen]
        dx = np.array([mv[1] for mv in moves])[chosen]
        r[w] += dy
        c[w] += dx
        for k, wi in enumerate(w):
            cells[wi].append(int(r[wi] * W + c[wi]))
        active[w] = ~gl[r[w], c[w]]
        j += 1
    return Routes(cells, csum, lsum, fragile, status)


def walk_many(planes, cost, goal, passable, groups, tau, mask, dtype=f64):
    """``walk`` for several groups of walkers of ONE map at once -- ``groups``: [(starts [n], u_of), ...] -> [Routes, ...] (a move of the
    walker is a handful of numpy calls whatever the number of walkers)"""
    sizes = [len(st) for st, _ in groups]
    r = walk(planes, cost, goal, passable, np.concatenate([np.asarray(st, np.int64) for st, _ in groups]), tau, mask,
             lambda j: np.concatenate([np.asarray(u_of(j), f64) for _, u_of in groups]), dtype)
    cuts = np.cumsum([0] + sizes)
    return [Routes(r.cells[a:b], r.cost[a:b], r.log_prob[a:b], r.fragile[a:b], r.status[a:b]) for a, b in zip(cuts, cuts[1:])]


def recursion_planes(dists_by_horizon, goal, passable):
    """the kernel's fields ``dists`` of horizons 1 .. K-1 (each [H,W]: 0 on EVERY goal) -> the planes [V_0 .. V_{K-1}] as the recursion
    reads them: +inf on obstacles, a goal on an obstacle too; V_0 is 0 on the passable goals and +inf elsewhere"""
    gl, ok = np.asarray(goal) != 0, np.asarray(passable) != 0
    V0 = np.where(gl & ok, 0.0, np.inf)
    return [V0] + [np.where(ok, np.asarray(d, f64), np.inf) for d in dists_by_horizon]


def visits(cells, HW: int) -> np.ndarray:
    """[HW] int64: how often the routes stood on each cell, every route's last cell not counted"""
    out = np.zeros(HW, np.int64)
    for route in cells:
        np.add.at(out, np.asarray(route[:-1], np.int64), 1)
    return out


def padded(cells, cap: int) -> np.ndarray:
    """the rows of routes_out: the LAST min(len, cap) cells of each route, then -1"""
    out = np.full((len(cells), cap), -1, np.int32)
    for k, route in enumerate(cells):
        keep = route[max(0, len(route) - cap):]
        out[k, :len(keep)] = keep
    return out


# ---- the bounds the GPU tests hold the kernel to ---------------------------------------------------------------------------------------------
# log_probs against (dists[start] - route_costs) / tau, relative to the case's scale max(1, max|V| / tau) (the size of the two quotients
# whose difference it is; 1 where the field is smaller than tau).  Measured on the cases of tests/test_soft_routes_gpu.py:
#   float32 stand-in (float32 planes of tests/soft_fields_oracle.py, the draw in float32; tests/test_soft_routes.py prints it)   LOGP_STANDIN
#   kernels (MI355X, the worst case of test_routes_are_the_oracles)                                                               LOGP_KERNELS
# The bound is 4 x the larger of the two, the rule of soft_fields_oracle.FWD_RTOL and for its reason: the figure is the float32 PLANES' --
# log p telescopes to (V_K(n_0) - cost) / tau only as exactly as every V_k(n) is cost[n] + softmin of V_{k-1}, which a float32 plane is to
# a few 2^-24 |V|, divided by tau, once per move -- and 4 x is headroom for another machine's exp2 and log, not for a wrong kernel.
LOGP_STANDIN = 8.18e-06
LOGP_KERNELS = 3.04e-06
LOGP_RTOL = 4 * max(LOGP_STANDIN, LOGP_KERNELS)
# the share of fragile routes, the worst case: float32 stand-in / kernels (the bound is FRAGILE_MAX_SHARE)
FRAGILE_MEASURED = (0.0313, 0.0313)


# ---- the cases the CPU and the GPU tests share ---------------------------------------------------------------------------------------------------
# (H, W, B, seed) of soft_fields_oracle.SHAPE_CASES: a goal alone; one row, one column; fewer cells than a wavefront with B = 3 and an odd
# H*W; 256 cells, the most the 64-lane workgroup takes; 1023 cells, the 256-lane workgroup.  BIG_CASE: 12288 cells, the limit and the
# 1024-lane workgroup, run once: the default horizon 448, Moore-8, tau = 0.02 and twelve goals.  (At tau = 1.0 the entropy outweighs costs
# of U(0.1, 1): a route then spends ALL K moves before it enters a goal -- 129 cells on the 31x33 maps, where 3.6 % of the routes are
# fragile -- and on this map V reaches -680 and 58 % of the 449-cell routes make a fragile draw somewhere: the case would say nothing.  At
# 0.02 the routes are under twenty cells and 0.5 % are fragile.)
SHAPE_CASES = ((1, 1, 1, 1), (1, 9, 1, 2), (9, 1, 1, 3), (5, 7, 3, 4), (16, 16, 2, 7), (31, 33, 3, 5))
BIG_CASE = (96, 128, 1, 9)
# (S, N): 1, 15, 64, 65 walkers per map -- below, at and one past a wavefront -- and 300: more than one workgroup of either kernel shape up
# to 1024 cells (64 or 256 lanes streaming, 256 gathering).  BIG_WALKERS: 1200, more than the one 1024-lane workgroup of the big map.
WALKERS = ((1, 1), (3, 5), (2, 32), (5, 13), (4, 75))
BIG_WALKERS = (2, 600)


def case_maps(H, W, B, seed):
    """cost, passable, goal [B,H,W] float32: soft_fields_oracle.random_maps; the big case gets eleven more goals on passable cells"""
    import soft_fields_oracle as SO
    cost, passable, goal = SO.random_maps(seed, B, H, W)
    if (H, W) == BIG_CASE[:2]:
        rng = np.random.default_rng(seed + 1000)
        free = np.flatnonzero(passable[0].reshape(-1) != 0)
        goal[0].reshape(-1)[rng.choice(free, 11, replace=False)] = 1
    return cost, passable, goal


def case_starts(seed, S, passable, goal) -> np.ndarray:
    """[B,S] int32 flat start cells: random cells of the whole map (obstacles too); the first on a passable cell; with S >= 3 the second
    on a goal and the third alternately one below and one past the map"""
    B, H, W = passable.shape
    rng = np.random.default_rng(seed)
    st = rng.integers(0, H * W, (B, S)).astype(np.int32)
    for b in range(B):
        st[b, 0] = rng.choice(np.flatnonzero(passable[b].reshape(-1) != 0))
        if S >= 3:
            st[b, 1] = rng.choice(np.flatnonzero(goal[b].reshape(-1) != 0))
            st[b, 2] = -1 if b % 2 == 0 else H * W
    return st


def cases(H, W, B, seed):
    """(K, tau, mask, (S, N), sample seed) of one shape: every (horizon, tau, mask) of soft_fields_oracle.sweep_cases, the walker counts
    taken in turn so that each count meets each shape"""
    import soft_fields_oracle as SO
    _, passable, goal = case_maps(H, W, B, seed)
    big = (H, W) == BIG_CASE[:2]
    sweep = [(2 * (H + W), 0.02, MOORE8)] if big else list(SO.sweep_cases(goal[0], passable[0]))
    for k, (K, tau, mask) in enumerate(sweep):
        yield K, tau, mask, (BIG_WALKERS if big else WALKERS[(k + seed) % len(WALKERS)]), 1000 * seed + k


def oracle_cases(H, W, B, seed):
    """(K, tau, mask, [((S, N), sample seed), ...]) of one shape for the comparison with the walker: every (horizon, tau, mask) with EVERY
    walker count.  The share of fragile routes is taken over all the routes of such a case -- a count of 1 or 15 walkers has too few
    routes for a share of 5 % to mean anything."""
    import soft_fields_oracle as SO
    _, passable, goal = case_maps(H, W, B, seed)
    if (H, W) == BIG_CASE[:2]:
        yield 2 * (H + W), 0.02, MOORE8, [(BIG_WALKERS, 1000 * seed)]
        return
    for k, (K, tau, mask) in enumerate(SO.sweep_cases(goal[0], passable[0])):
        yield K, tau, mask, [(sn, 1021 * seed + 10 * k + n) for n, sn in enumerate(WALKERS)]


def case_uniforms(sample_seed, B, S, N):
    """u_of(j) -> [B*S*N] for the walkers of a batch in (b, s, i) order, from Philox as the header says"""
    q, i = np.repeat(np.arange(B * S), N), np.tile(np.arange(N), B * S)
    return lambda j: uniform(sample_seed, q, i, j)


def crafted_uniforms(sample_seed, B, S, N, K) -> np.ndarray:
    """[B,S,N,K] float32 for the ``uniforms`` argument: random rows, and the crafted rows u = 0 (sample 0) and u -> 1 (sample 1)"""
    uni = np.random.default_rng(sample_seed).random((B, S, N, K)).astype(f32)
    uni[:, :, 0] = 0
    if N > 1:
        uni[:, :, 1] = 1 - 2.0 ** -24
    return uni


def logp_scale(planes, tau: float) -> float:
    fin = np.asarray(planes[-1], f64)
    fin = np.abs(fin[np.isfinite(fin)])
    return max(1.0, float(fin.max()) / tau) if fin.size else 1.0
