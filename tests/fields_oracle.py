"""The cost-to-go field and its optimal policy in numpy: the DEFINITION of include/nastar_fields.h.

A move n -> m = n + off, off in ``heuristic_oracle.offsets(mask)``, m inside the map and passable, costs cost[n] (the cell being left).
D(goal) = 0; D(n) = min over the moves of fl32(cost[n] + D(m)), found by a Jacobi relaxation in fp32 from "+inf everywhere but the goals"
to the fixed point; +inf on non-goal obstacles and where no goal can be reached.  A goal on an obstacle is 0 and cannot be entered.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from heuristic_oracle import MOORE8, offsets  # noqa: E402

f32 = np.float32
ACTION_MOVES = ((-1, 0), (0, 1), (0, -1), (1, 0), (-1, 1), (-1, -1), (1, 1), (1, -1))  # synthetic.ACTION_MOVES
STATUS_OK, STATUS_NO_GOAL, STATUS_BAD_COST = 0, 3, 9


def _shifted(x, dy, dx):
    """y[r, c] = x[r + dy, c + dx], +inf outside the map"""
    H, W = x.shape
    pad = np.full((H + 2, W + 2), np.inf, f32)
    pad[1:-1, 1:-1] = x
    return pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def field(cost, goal, passable, mask=MOORE8, want_sweeps=False):
    """[H,W] arrays -> (D [H,W] f32, policy [8,H,W] f32, status)"""
    cost, ok, goal = np.asarray(cost, f32), np.asarray(passable) != 0, np.asarray(goal) != 0
    H, W = cost.shape
    inf = np.full((H, W), np.inf, f32)
    zero = np.zeros((8, H, W), f32)
    if (ok & ~(cost >= 0)).any():
        return inf, zero, STATUS_BAD_COST
    moves = offsets(mask)
    r = np.where(goal & ok, f32(0), inf)  # what a move may read: an obstacle (a goal on one too) is never entered
    sweeps = 0
    with np.errstate(invalid="ignore"):
        while True:
            nb = np.min([_shifted(r, dy, dx) for dy, dx in moves], axis=0) if moves else inf
            new = np.where(ok, np.minimum(r, (cost + nb).astype(f32)), inf)
            sweeps += 1
            if np.array_equal(new, r):
                break
            r = new
    d = np.where(goal, f32(0), r)
    pol = zero.copy()
    best, arg = inf.copy(), np.full((H, W), -1)
    for k, (dy, dx) in enumerate(ACTION_MOVES):
        if (dy, dx) in moves:
            v = _shifted(r, dy, dx)
            arg = np.where(v < best, k, arg)
            best = np.minimum(best, v)
    pick = np.isfinite(r) & (r > 0) & (best < r)
    rr, cc = np.nonzero(pick)
    pol[arg[rr, cc], rr, cc] = 1
    out = (d, pol, STATUS_OK if goal.any() else STATUS_NO_GOAL)
    return out + (sweeps,) if want_sweeps else out


def fields(cost, goal, passable, mask=MOORE8):
    """[B,(1,)H,W] arrays -> (D [B,H,W], policies [B,8,H,W], status [B] int32)"""
    c, g, p = (np.asarray(a).reshape((a.shape[0],) + a.shape[-2:]) for a in (cost, goal, passable))
    out = [field(c[b], g[b], p[b], mask) for b in range(c.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], np.int32)
