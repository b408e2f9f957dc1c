"""Ordered optimal routes for many start cells per map in numpy: the DEFINITION of include/nastar_field_routes.h.

The successor s(n) is that of ``fields_grad_oracle`` / ``fields_grad_tiled_oracle.forest``, by the header's words and from ``dist``, ``goal``
and ``passable`` alone: the FIRST action, in ``fields_oracle.ACTION_MOVES`` order, among the allowed in-map moves whose target has the
smallest READABLE value (dist where passable, +inf elsewhere), taken only if that value is strictly below dist[n]; a cell whose dist is not
below +inf has none.  (Vectorised here, so that a map of 164025 cells takes a moment; tests/test_field_routes.py pins it on both oracles.)
The route of a start n0 is n0, s(n0), s(s(n0)), ... up to and including the first goal cell.
"""
import os
import sys
from typing import NamedTuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fields_oracle as FO  # noqa: E402
from heuristic_oracle import MOORE8, offsets  # noqa: E402

f32 = np.float32
STATUS_OK, STATUS_BAD_SHAPE, STATUS_UNSOLVABLE, STATUS_PLATEAU = 0, 1, 3, 11


def successors(dist, goal, passable, mask=MOORE8) -> np.ndarray:
    """[H,W] arrays -> [H*W] int64: the flat index of s(n), -1 where there is none (goal cells are given theirs like any other cell: the
    chase never asks)"""
    d = np.asarray(dist, f32)
    H, W = d.shape
    readable = np.where(np.asarray(passable) != 0, d, f32(np.inf)).astype(f32)
    allowed = set(offsets(mask))
    best = np.full((H, W), np.inf, f32)
    step = np.zeros((H, W), np.int64)
    with np.errstate(invalid="ignore"):
        for dy, dx in FO.ACTION_MOVES:
            if (dy, dx) in allowed:
                v = FO._shifted(readable, dy, dx)
                better = v < best                       # strict: the first among equals stays
                best, step = np.where(better, v, best), np.where(better, dy * W + dx, step)
        has = (d < np.inf) & (best < d)
    return np.where(has, np.arange(H * W).reshape(H, W) + step, -1).reshape(-1)


def route(dist, goal, succ, n0):
    """-> (cells of the route of start n0, status); the cells are [] for a failed query"""
    d, g = np.asarray(dist, f32).reshape(-1), np.asarray(goal).reshape(-1)
    if not 0 <= n0 < d.size:
        return [], STATUS_BAD_SHAPE
    if not np.isfinite(d[n0]):
        return [], STATUS_UNSOLVABLE
    cells, n = [int(n0)], int(n0)
    while g[n] == 0:
        n = int(succ[n])
        if n < 0:
            return [], STATUS_PLATEAU
        cells.append(n)
        assert len(cells) <= d.size, "s strictly lowers dist: a route has at most H*W cells"
    return cells, STATUS_OK


class Routes(NamedTuple):
    routes: np.ndarray    # [S,L] int32: the last min(len, L) cells, the goal last, then -1
    lengths: np.ndarray   # [S] int32: the true lengths
    costs: np.ndarray     # [S] f32: dist[n0]; +inf outside the map
    status: np.ndarray    # [S] int32
    cells: list           # per start: the whole route


def routes(dist, goal, passable, starts, mask=MOORE8, cap=None) -> Routes:
    """[H,W] arrays and S flat start indices -> Routes; ``cap`` None: L = the longest route (at least 1)"""
    d = np.asarray(dist, f32)
    succ = successors(d, goal, passable, mask)
    out = [route(d, goal, succ, int(n0)) for n0 in starts]
    lengths = np.array([len(c) for c, _ in out], np.int32)
    L = max(1, int(lengths.max(initial=0))) if cap is None else cap
    rows = np.full((len(out), L), -1, np.int32)
    for s, (c, _) in enumerate(out):
        kept = c[len(c) - min(len(c), L):]
        rows[s, :len(kept)] = kept
    costs = np.array([d.reshape(-1)[n0] if 0 <= n0 < d.size else np.inf for n0 in starts], f32)
    return Routes(rows, lengths, costs, np.array([st for _, st in out], np.int32), [c for c, _ in out])


def batch(dist, goal, passable, starts, mask=MOORE8, cap=None):
    """[B,H,W] arrays and [B,S] starts -> (routes [B,S,L], lengths, costs, status) with one L for the batch"""
    per = [routes(dist[b], goal[b], passable[b], starts[b], mask, cap) for b in range(len(dist))]
    L = max(r.routes.shape[1] for r in per)
    rows = np.full((len(per), len(starts[0]), L), -1, np.int32)
    for b, r in enumerate(per):
        rows[b, :, :r.routes.shape[1]] = r.routes
    return rows, np.stack([r.lengths for r in per]), np.stack([r.costs for r in per]), np.stack([r.status for r in per])
