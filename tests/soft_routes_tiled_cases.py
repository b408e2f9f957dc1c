"""The cases tests/test_soft_routes_tiled.py (CPU) and tests/test_soft_routes_tiled_gpu.py share: sampled routes from the tiled soft field's
checkpointed tape (include/nastar_soft_routes_tiled.h), and the figures measured on them.

Above the one-workgroup limit there is no second kernel to compare bits with: the routes are held to the float64 walker of
tests/soft_routes_oracle.py, every route it does not flag fragile cell for cell, at most ``RO.FRAGILE_MAX_SHARE`` flagged (5 %, the
project's cap: a condition, not a measurement).

Measured on the cases below (``above_cases``; 600 walkers per map from Philox, sample seed ``SAMPLE_SEED``, the starts of
``above_starts``), float32 stand-in (``RO.walk(dtype=float32)`` on the float32 planes of tests/soft_fields_oracle.py;
tests/test_soft_routes_tiled.py prints it) and kernels (MI355X, tests/test_soft_routes_tiled_gpu.py prints them) alike, flag for flag: no
mismatch outside the fragile band anywhere.  The fragile shares, stand-in / kernels:
    48x130, K = 60    Moore-8 tau 0.05: 1.14 % / 1.14 %, tau 0.5: 0.95 % / 0.95 %;  0x0AA tau 0.05: 1.24 % / 1.24 %, tau 0.5: 0.48 % / 0.48 %
    130x140, K = 97   Moore-8 tau 0.05: 4.22 % / 4.22 % (19 of 450 routes: the worst), tau 0.5: 0.67 % / 0.67 %;  0x0AA: 1.11 % / 1.11 % at both
The starts are drawn within K hops under the case's own move set -- drawn under Moore-8, both near starts of the 130x140 map are out of
reach of the 4-connected walker and the case says nothing -- so the draws, and with them the shares, are not those of the issue that asked
for this (2.7 % at worst): these are the figures of the committed seeds, re-checked on the stand-in before the kernels ran.
The log-prob gaps on 130x140, relative to ``RO.logp_scale``: stand-in 1.9e-07, 1.3e-07, 1.3e-07, 2.2e-07; kernels 2.2e-07, 2.2e-07, 1.1e-07,
2.8e-07 (Moore-8 tau 0.05, 0.5, then 0x0AA).
"""
import functools

import numpy as np

import soft_fields_oracle as SO
import soft_fields_tiled_cases as TC
import soft_routes_oracle as RO

f32, f64 = np.float32, np.float64

ABOVE, ABOVE_MASKS = TC.ABOVE, TC.ABOVE_MASKS
ABOVE_TAUS = (0.05, 0.5)
ABOVE_S, ABOVE_N = 4, 150          # 600 walkers per map: more than one 256-lane workgroup
SAMPLE_SEED = 12345


@functools.lru_cache(maxsize=None)
def above_starts(H, W, B, seed, K, mask=SO.MOORE8) -> np.ndarray:
    """[B,4] int32 from ``default_rng(7000 + seed + b)``: two passable cells within K hops of the goal under ``mask`` (no goals), one goal,
    one cell anywhere on the map (an obstacle or a cell out of reach among them)"""
    _, passable, goal = TC.maps(H, W, B, seed)
    st = np.zeros((B, ABOVE_S), np.int32)
    for b in range(B):
        rng = np.random.default_rng(7000 + seed + b)
        hops = SO.hops(goal[b], passable[b], mask).reshape(-1)
        st[b, :2] = rng.choice(np.flatnonzero((hops > 0) & (hops <= K)), 2, replace=False)
        st[b, 2] = rng.choice(np.flatnonzero(goal[b].reshape(-1) != 0))
        st[b, 3] = rng.integers(0, H * W)
    return st


def above_cases():
    """(H, W, B, seed, K, tau, mask) of every comparison with the oracle above the one-workgroup limit"""
    for H, W, B, seed, K in ABOVE:
        for mask in ABOVE_MASKS:
            for tau in ABOVE_TAUS:
                yield H, W, B, seed, K, tau, mask


def above_groups(b, starts, B):
    """the walkers of map b as ``RO.walk_many`` takes them: [(starts [S*N], u_of)] with Philox's uniforms"""
    S, N = ABOVE_S, ABOVE_N
    u = RO.case_uniforms(SAMPLE_SEED, B, S, N)
    sel = slice(b * S * N, (b + 1) * S * N)
    return [(np.repeat(starts[b], N), lambda j: u(j)[sel])]


# the share of fragile routes, the worst of ``above_cases``: float32 stand-in, kernels (the bound is RO.FRAGILE_MAX_SHARE)
STANDIN_FRAGILE, KERNELS_FRAGILE = 0.0423, 0.0423
# log_probs against (dists[start] - route_costs) / tau on the 130x140 case, relative to RO.logp_scale, the worst of its taus and masks:
# float32 stand-in (CPU), kernels (MI355X); the bound is 4 x the larger, as RO.LOGP_RTOL is formed and for its reason
LOGP_STANDIN, LOGP_KERNELS = 2.23e-07, 2.79e-07
LOGP_RTOL = 4 * max(LOGP_STANDIN, LOGP_KERNELS)

# ---- visits / N against the tiled backward: map 0 of soft_fields_tiled_cases.maxent_maps(), the start 40 hops from the goal -----------------------
VISITS_TAU, VISITS_N, VISITS_SEED = 0.5, 4096, 3


def visits_bound(per, expect, N, tol):
    """the bound on |visits / N - expect| per cell: 5 standard errors plus ``tol`` (the backward's tolerance), the rule of
    tests/test_soft_routes_gpu.py.  ``per`` [N,HW]: the visits of each route.  The standard error of a cell is the larger of the sample's
    and sqrt(p (1 - p) / N) with p = expect (where that is below 1): a route's visit count X is a non-negative integer, so E[X^2] >= E[X] and
    Var X >= p - p^2 -- the sample's own figure is 0 on a cell none of the N routes stood on, which on these maps (the routes wander for all
    K = 97 moves at tau 0.5, and thousands of cells expect fewer than 1 / N visits) would hold those cells to ``tol`` alone: the float64
    oracle itself misses that on 24 to 58 cells, whatever the seed."""
    p = np.asarray(expect, f64)
    se = np.maximum(per.astype(f64).std(0, ddof=1), np.sqrt(np.maximum(p - p * p, 0.0))) / np.sqrt(N)
    return 5 * se + tol


# ---- the far corner: soft_fields_tiled_cases' 1024 x 1152 map, 64 samples from CORNER_START and 64 from the last cell -----------------------------
CORNER_N, CORNER_SEED = 64, 21
CORNER_STARTS = (TC.CORNER_START[0] * TC.CORNER_W + TC.CORNER_START[1], TC.CORNER_H * TC.CORNER_W - 1)


def corner_maps():
    """``soft_fields_tiled_cases.corner_maps()`` with the map's last cell passable (there it is an obstacle): the walker that starts on
    cell H*W - 1 is two moves from the goal"""
    cost, passable, goal = (a.copy() for a in TC.corner_maps())
    passable[0, -1, -1] = 1
    return cost, passable, goal
