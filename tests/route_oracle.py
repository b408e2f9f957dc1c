"""Ordered routes, their lengths and float64 costs in numpy: the checker of ``plan_routes()``.

Built on ``heuristic_oracle._Map`` (the per-map state, ``step()``, ``parent``); it restates that module's two driver loops -- early exit
(every map stops at the step that selects its goal) and lock-step (the reference's batch loop) -- because the route needs the parents the
loop leaves behind, which ``heuristic_oracle.search`` does not return.

The route of a map is the walk of ``_Map.path(t)`` -- the goal, then at most t hops along the parents from the goal's parent, ending at the
start or back at the goal (a parent that still holds its initial value) -- as a LIST, reversed: travel order, the goal last.
``tests/test_routes.py`` pins it on the CPU against every golden ``paths`` mask.
"""
from __future__ import annotations

from typing import List, NamedTuple

import numpy as np

import heuristic_oracle as HO

f32 = np.float32


class Routes(NamedTuple):
    routes: List[List[int]]   # per map: flat cell indices in travel order, the goal last ([] = no one-hot goal)
    lengths: np.ndarray       # [B] int32
    costs: np.ndarray         # [B] float64: sum of cost over the route cells except the goal
    histories: np.ndarray     # [B,H,W] f32
    paths: np.ndarray         # [B,H,W] i64
    status: np.ndarray        # [B]
    reached: np.ndarray       # [B] bool: the map's search selected its goal


def builtin_h0(goal_maps) -> np.ndarray:
    """the reference's get_heuristic for one-hot goal maps [B,(1,)H,W] -> [B,H,W] (the oracle's, bit-exact with the kernels')"""
    from oracle import oracle as O
    goal = np.asarray(goal_maps).reshape((goal_maps.shape[0],) + goal_maps.shape[-2:])
    B, H, W = goal.shape
    out = np.zeros((B, H, W), f32)
    for b in range(B):
        nz = np.flatnonzero(goal[b].reshape(-1))
        out[b] = O.heuristic(H, W, *divmod(int(nz[-1]) if nz.size else 0, W))
    return out


def route_of(m: "HO._Map", t: int) -> List[int]:
    """``_Map.path(t)`` as an ordered list (goal last)"""
    if m.goal < 0:
        return []
    cells = [m.goal]
    loc = int(m.parent[m.goal])
    for _ in range(t):
        if loc == m.goal:
            break
        cells.append(loc)
        if loc == m.start:
            break
        loc = int(m.parent[loc])
    return cells[::-1]


def plan(cost, start, goal, passable, g_ratio: float, max_iters: int, mask: int = HO.MOORE8, h0=None, lockstep: bool = False) -> Routes:
    """[B,(1,)H,W] arrays.  ``h0`` None = the built-in heuristic.  ``lockstep``: the reference's batch loop (what the module runs for a batch
    of more than one map when g_ratio is outside [0.5, 1) or a heuristic is given), else every map on its own."""
    if h0 is None:
        h0 = builtin_h0(goal)
    cost, start, goal, passable, h0 = (np.asarray(a).reshape((a.shape[0],) + a.shape[-2:]) for a in (cost, start, goal, passable, h0))
    B, H, W = cost.shape
    maps = [HO._Map(cost[b], start[b], goal[b], passable[b], h0[b], g_ratio, mask) for b in range(B)]
    live = [m.status == 0 for m in maps]

    def alone(m):
        while len(m.sel) < max_iters:
            s = m.step()
            if s < 0 or s == m.goal:
                break

    if not lockstep:
        for b, m in enumerate(maps):
            if live[b]:
                alone(m)
    else:
        # (a map without a route takes no part in the batch loop: it is searched alone, heuristic_oracle.search)
        probe = [HO._Map(cost[b], start[b], goal[b], passable[b], h0[b], g_ratio, mask) for b in range(B)]
        for b, p in enumerate(probe):
            if live[b]:
                alone(p)
            if p.status != 0:
                live[b] = False
                maps[b] = p
        for _ in range(max_iters):
            all_goal, any_live = True, False
            for b, m in enumerate(maps):
                if not live[b]:
                    continue
                s = m.step()
                if s < 0:
                    live[b] = False
                    continue
                any_live = True
                all_goal &= s == m.goal
            if not any_live or all_goal:
                break
    routes = [route_of(m, max(len(m.sel) - 1, 0)) for m in maps]
    costs = np.array([sum(float(m.cost[c]) for c in r[:-1]) for m, r in zip(maps, routes)], np.float64)
    return Routes(routes, np.array([len(r) for r in routes], np.int32), costs,
                  np.stack([m.hist.reshape(H, W).astype(f32) for m in maps]),
                  np.stack([m.path(max(len(m.sel) - 1, 0)).reshape(H, W) for m in maps]),
                  np.array([m.status for m in maps], np.int32), np.array([bool(m.sel) and m.goal in m.sel for m in maps]))


def rows(r: Routes, cap: int) -> np.ndarray:
    """the [B, cap] int32 tensor ``plan_routes`` returns: the last min(len, cap) cells of every route, then -1"""
    out = np.full((len(r.routes), cap), -1, np.int32)
    for b, cells in enumerate(r.routes):
        keep = cells[-cap:] if cells else []
        out[b, :len(keep)] = keep
    return out
