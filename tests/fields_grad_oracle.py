"""The gradient of the cost-to-go field with respect to the cost maps in numpy float64: the DEFINITION of include/nastar_fields_grad.h
(DESIGN.md section 2, item 6g), on top of ``fields_oracle.field``.

The successor s(n) of a live cell (not a goal, finite D) is the action ``fields_oracle.field`` gives it -- the first action among the allowed
moves whose target has the smallest readable value r, if that is strictly below D(n).  dD(n)/dcost[v] = 1 for v on the roll-out from n, so
grad_cost[v] = A(v) = G(v) + sum of A(c) over the live c with s(c) = v: the live cells are visited in DECREASING D (a child before its
parent: s strictly lowers D) and each adds its A into its successor.  G is read on live cells only.  A live cell without a successor
(a zero-cost plateau) fails its map: status 11, all zeros.
"""
import os
import sys
from typing import NamedTuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fields_oracle as FO  # noqa: E402
from heuristic_oracle import MOORE8  # noqa: E402

f32 = np.float32
STATUS_OK, STATUS_PLATEAU = 0, 11


class FieldGrad(NamedTuple):
    grad: np.ndarray    # [H,W] f32: fl32(A) on live cells, 0 elsewhere
    A: np.ndarray       # [H,W] f64: the sums before the rounding (0 where not live)
    status: int         # 0 or 11
    live: np.ndarray    # [H,W] bool
    succ: np.ndarray    # [H,W] flat index of s(n) on live cells (-1 elsewhere, and on a live cell without a successor)
    hops: np.ndarray    # [H,W] moves from the cell to its goal along s (0 where not live)
    dist: np.ndarray    # [H,W] f32: the field


def field_grad(cost, goal, passable, G, mask=MOORE8) -> FieldGrad:
    """[H,W] arrays -> FieldGrad"""
    d, pol, _ = FO.field(cost, goal, passable, mask)
    H, W = d.shape
    live = (np.asarray(goal) == 0) & np.isfinite(d)
    has = pol.sum(0) > 0
    act = pol.argmax(0)
    succ = np.full((H, W), -1, np.int64)
    for y, x in np.argwhere(live & has):
        dy, dx = FO.ACTION_MOVES[act[y, x]]
        succ[y, x] = (y + dy) * W + (x + dx)
    zeros = np.zeros((H, W))
    if (live & ~has).any():
        return FieldGrad(zeros.astype(f32), zeros, STATUS_PLATEAU, live, succ, np.zeros((H, W), np.int64), d)
    A = np.where(live, np.asarray(G, np.float64), 0.0)  # (where, not a product: a NaN on a cell that is not live is never read)
    flat_live, flat_succ, Af = live.reshape(-1), succ.reshape(-1), A.reshape(-1)
    order = np.argsort(-d.reshape(-1), kind="stable")
    order = order[flat_live[order]]
    for n in order:             # decreasing D: every child of a cell has been added before the cell is
        s = flat_succ[n]
        if flat_live[s]:        # (the successor of a root is a goal: nothing to add into)
            Af[s] += Af[n]
    hops = np.zeros(H * W, np.int64)
    for n in order[::-1]:       # increasing D: a cell's successor has its count
        hops[n] = hops[flat_succ[n]] + 1
    return FieldGrad(np.where(live, A, 0.0).astype(f32), A, STATUS_OK, live, succ, hops.reshape(H, W), d)


def field_grads(cost, goal, passable, G, mask=MOORE8):
    """[B,(1,)H,W] arrays -> [FieldGrad] * B"""
    c, g, p, u = (np.asarray(a).reshape((a.shape[0],) + a.shape[-2:]) for a in (cost, goal, passable, G))
    return [field_grad(c[b], g[b], p[b], u[b], mask) for b in range(c.shape[0])]
