"""A numpy restatement of the search WITH THE HEURISTIC AS AN INPUT, and the loader of tests/golden/heuristics/*.npz.

``oracle/`` computes h0 itself; the kernels behind ``forward(..., heuristic_maps=)`` take it from the caller.  This module states the
algorithm of DESIGN.md section 2 once more, in numpy, with ``h0`` as an argument:

  * state per cell: g, open, closed (= histories), parent; the open list starts as {start} with g = 0, parents start at the goal;
  * a step selects the open cell with the smallest ``q = fl(f / fl32(sqrt(W)))``, ``f = fl(fl(g_ratio g) + fl((1 - g_ratio) fl(h0 + cost)))``
    (fp32, one rounding per operation), the first flat index on ties (the quotient rule, item 5);
  * the selected cell s joins histories and leaves the open list -- unless it is the goal, which stays open; ``g2 = fl(g[s] + cost[s])``;
    every neighbour n the 9-bit mask opens (bit r*3+c <=> filter cell (r, c); filter cell (a, b) opens offset (1-a, 1-b)), inside the map and
    passable, with ((not open and not in histories) or (open and g[n] > g2)) gets g = g2, parent = s and is open;
  * ``lockstep=False``: every map stops at the step that selects its goal (what one map searched alone does);
    ``lockstep=True``: the batch loop -- every map is stepped until ALL maps select their goal in the same step, or the budget ends
    (a map without a route is reported and takes no part in it);
  * paths: the goal, then t hops along the parents from the goal's parent (t = index of the map's last step).

``tests/test_heuristic_oracle.py`` pins it on the CPU: every reference vector, and ``oracle.forward()`` on Moore-8 vectors.
"""
from __future__ import annotations

import glob
import math
import os
from typing import List, NamedTuple, Optional

import numpy as np

f32 = np.float32
DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "heuristics")
MOORE8 = 0x1EF
VON_NEUMANN = 0x0AA
STATUS_UNSOLVABLE = 3


def offsets(mask: int):
    return [(1 - a, 1 - b) for a in range(3) for b in range(3) if (mask >> (a * 3 + b)) & 1]


class _Map:
    def __init__(self, cost, start, goal, passable, h0, g_ratio, mask):
        self.H, self.W = cost.shape
        HW = self.H * self.W
        self.cost = np.ascontiguousarray(cost, f32).reshape(-1)
        self.passable = passable.reshape(-1) != 0
        self.gr, omg = f32(g_ratio), f32(1.0 - g_ratio)
        self.sq = f32(math.sqrt(self.W))
        self.hh = (omg * (np.ascontiguousarray(h0, f32).reshape(-1) + self.cost)).astype(f32)  # fl(omg * fl(h0 + cost))
        self.moves = offsets(mask)
        s = np.flatnonzero(start.reshape(-1))
        g = np.flatnonzero(goal.reshape(-1))
        self.status = 0 if (s.size and g.size) else STATUS_UNSOLVABLE
        self.start = int(s[-1]) if s.size else -1
        self.goal = int(g[-1]) if g.size else -1
        self.g = np.zeros(HW, f32)
        self.open = np.zeros(HW, bool)
        self.hist = np.zeros(HW, bool)
        self.q = np.full(HW, np.inf, f32)      # q of the open cells, +inf elsewhere
        self.parent = np.full(HW, self.goal, np.int64)
        self.sel: List[int] = []
        if self.status == 0:
            self._open(self.start, f32(0.0))

    def _open(self, n, g):
        self.g[n] = g
        self.open[n] = True
        f = f32(f32(self.gr * g) + self.hh[n])
        self.q[n] = f32(f / self.sq)

    def step(self) -> int:
        """one step; returns the selected cell, or -1 when the open list is empty (the map is then unsolvable)"""
        if not self.open.any():
            self.status = STATUS_UNSOLVABLE
            return -1
        s = int(np.argmin(self.q))  # first flat index of the minimum
        self.sel.append(s)
        self.hist[s] = True
        if s != self.goal:
            self.open[s] = False
            self.q[s] = np.inf
        g2 = f32(self.g[s] + self.cost[s])
        r, c = divmod(s, self.W)
        for dr, dc in self.moves:
            nr, nc = r + dr, c + dc
            if not (0 <= nr < self.H and 0 <= nc < self.W):
                continue
            n = nr * self.W + nc
            if not self.passable[n]:
                continue
            if (not self.open[n] and not self.hist[n]) or (self.open[n] and self.g[n] > g2):
                self._open(n, g2)
                self.parent[n] = s
        return s

    def path(self, t: int) -> np.ndarray:
        p = np.zeros(self.H * self.W, np.int64)
        if self.goal < 0:
            return p
        p[self.goal] = 1
        loc = int(self.parent[self.goal])
        for _ in range(t):
            if p[loc] and loc == self.goal:
                break  # (the goal's parent is still the initial value: the walk stays on the goal)
            p[loc] = 1
            if loc == self.start:
                break  # (the start's parent is the initial value, the goal: the walk would repeat itself)
            loc = int(self.parent[loc])
        return p


class Result(NamedTuple):
    histories: np.ndarray   # [B,H,W] f32
    paths: np.ndarray       # [B,H,W] i64
    sel: list               # per map: the cell selected at every step it executed
    iters: np.ndarray       # [B] steps executed
    status: np.ndarray      # [B] 0 / STATUS_UNSOLVABLE
    t_batch: int            # index of the batch's last step


def search(cost, start, goal, passable, h0, g_ratio: float, max_iters: int, mask: int = MOORE8, lockstep: bool = False) -> Result:
    """[B,H,W] arrays (a channel axis of 1 is dropped).  ``lockstep``: see the module docstring."""
    cost, start, goal, passable, h0 = (np.asarray(a).reshape((a.shape[0],) + a.shape[-2:]) for a in (cost, start, goal, passable, h0))
    B, H, W = cost.shape
    maps = [_Map(cost[b], start[b], goal[b], passable[b], h0[b], g_ratio, mask) for b in range(B)]
    live = [m.status == 0 for m in maps]
    if lockstep:
        # The reference has no answer for a batch that holds a map without a route (it crashes); the package reports such a map and lets it take
        # NO part in the batch loop (include/nastar.h, nastar_forward_batchloop_finish): it is searched alone, the others are stepped together.
        alone = search(cost, start, goal, passable, h0, g_ratio, max_iters, mask, lockstep=False)
        for b in range(B):
            if alone.status[b] != 0:
                live[b] = False
                if maps[b].status == 0:
                    while maps[b].step() >= 0:
                        pass
    if not lockstep:
        for b, m in enumerate(maps):
            while live[b] and len(m.sel) < max_iters:
                s = m.step()
                if s < 0 or s == m.goal:
                    break
    else:
        for t in range(max_iters):
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
    iters = np.array([len(m.sel) for m in maps], np.int32)
    hist = np.stack([m.hist.reshape(H, W).astype(f32) for m in maps])
    paths = np.stack([m.path(max(len(m.sel) - 1, 0)).reshape(H, W) for m in maps])
    status = np.array([m.status for m in maps], np.int32)
    ok = status == 0
    return Result(hist, paths, [m.sel for m in maps], iters, status, int(iters[ok].max()) - 1 if ok.any() else -1)


# ---- the reference vectors of tools/gen_golden_heuristic.py ----------------------------------------------------------------------------
class HGolden(NamedTuple):
    name: str
    mask: int
    g_ratio: float
    Tmax: float
    training: bool
    map_designs: np.ndarray  # [B,1,H,W] f32
    start_maps: np.ndarray
    goal_maps: np.ndarray
    cost_maps: np.ndarray
    h0: np.ndarray           # [B,1,H,W] f32
    histories: np.ndarray
    paths: np.ndarray
    sel_log: np.ndarray      # [B, t_batch + 1]
    t_batch: int
    target: Optional[np.ndarray]
    grad_cost: Optional[np.ndarray]
    grad_h0: Optional[np.ndarray]
    h0_only: bool            # grad_* vectors: requires_grad on h0 only (cost maps == map designs, VanillaAstar)

    @property
    def max_iters(self) -> int:
        W = self.map_designs.shape[-1]
        return int((self.Tmax if self.training else 1.0) * W * W)


def names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(DIR, "*.npz")))


def _unpack(bits, B, H, W):
    return np.unpackbits(bits, axis=-1)[..., :H * W].reshape(bits.shape[:-1] + (1, H, W))


def load(name: str) -> HGolden:
    z = np.load(os.path.join(DIR, name + ".npz"))
    B, H, W = int(z["B"]), int(z["H"]), int(z["W"])
    maps = _unpack(z["map_bits"], B, H, W).astype(f32)
    eye = np.eye(H * W, dtype=f32)
    return HGolden(
        name=name, mask=int(z["mask"]), g_ratio=float(z["g_ratio"]), Tmax=float(z["Tmax"]), training=bool(z["training"]),
        map_designs=maps, start_maps=eye[z["start_idx"]].reshape(B, 1, H, W), goal_maps=eye[z["goal_idx"]].reshape(B, 1, H, W),
        cost_maps=z["cost"].astype(f32) if "cost" in z else maps, h0=z["h0"].astype(f32).reshape(B, 1, H, W),
        histories=_unpack(z["hist_bits"], B, H, W).astype(f32), paths=_unpack(z["path_bits"], B, H, W).astype(np.int64),
        sel_log=z["sel_log"], t_batch=int(z["t_batch"]),
        target=_unpack(z["target_bits"], B, H, W).astype(f32) if "target_bits" in z else None,
        grad_cost=z["grad_cost"] if "grad_cost" in z else None, grad_h0=z["grad_h0"] if "grad_h0" in z else None,
        h0_only=bool(z["h0_only"]) if "h0_only" in z else False,
    )
