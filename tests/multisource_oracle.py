"""A numpy restatement of the MULTI-SOURCE search and the loader of tests/golden/multisource/*.npz.

Built on ``heuristic_oracle._Map`` and different from it in exactly two places:

  * the open list starts as EVERY non-zero cell of the start map (the reference's ``open_maps = start_maps``), each with g = 0;
  * the parents start UNSET (-1 here; the reference's initial value is the goal index, which makes its literal t-hop walk run round the
    same chain again) and the path walk ends at the first cell whose parent is unset, or after t hops -- not "at the start".

Everything else -- keys, ties, steps, the lock-step batch loop, statuses -- is ``heuristic_oracle``'s, used as it is.
``tests/test_multisource.py`` pins this module on every reference vector.
"""
from __future__ import annotations

import glob
import os
from typing import NamedTuple, Optional

import numpy as np

import heuristic_oracle as HO

f32 = np.float32
DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multisource")
MOORE8 = HO.MOORE8
VON_NEUMANN = HO.VON_NEUMANN
STATUS_UNSOLVABLE = HO.STATUS_UNSOLVABLE
UNSET = -1


class _MultiMap(HO._Map):
    def __init__(self, cost, start, goal, passable, h0, g_ratio, mask):
        super().__init__(cost, start, goal, passable, h0, g_ratio, mask)
        self.sources = [int(s) for s in np.flatnonzero(np.asarray(start).reshape(-1))]
        self.parent = np.full(self.H * self.W, UNSET, np.int64)  # difference 2: unset, not "the goal"
        if self.status == 0:
            for s in self.sources:  # difference 1: every start is open with g = 0
                self._open(s, f32(0.0))

    def path(self, t: int) -> np.ndarray:
        p = np.zeros(self.H * self.W, np.int64)
        if self.goal < 0:
            return p
        p[self.goal] = 1
        loc = int(self.parent[self.goal])
        for _ in range(t):
            if loc == UNSET:
                break
            p[loc] = 1
            loc = int(self.parent[loc])
        return p

    def route(self, t: int) -> list:
        """the cells of ``path(t)`` in travel order, the goal last (a chain that returns to a cell it holds stops there)"""
        if self.goal < 0:
            return []
        chain = [self.goal]
        loc = int(self.parent[self.goal])
        for _ in range(t):
            if loc == UNSET or loc in chain:
                break
            chain.append(loc)
            loc = int(self.parent[loc])
        return chain[::-1]


def search(cost, start, goal, passable, h0, g_ratio: float, max_iters: int, mask: int = MOORE8, lockstep: bool = False, with_maps: bool = False):
    """``heuristic_oracle.search`` over ``_MultiMap``: same arguments, same ``Result``.  ``h0`` None = the reference's heuristic.
    ``with_maps``: also return the per-map states (parents, selections) -> (Result, [maps])."""
    cost, start, goal, passable = (np.asarray(a).reshape((a.shape[0],) + a.shape[-2:]) for a in (cost, start, goal, passable))
    h0 = default_h0(goal) if h0 is None else np.asarray(h0).reshape(cost.shape)
    keep = []

    class Recording(_MultiMap):
        def __init__(self, *a):
            super().__init__(*a)
            keep.append(self)

    saved = HO._Map
    HO._Map = Recording  # (search() builds its maps through the module attribute; restored below)
    try:
        if lockstep:
            # heuristic_oracle.search runs the maps alone first (to find those without a route); only the batch run's states are wanted
            res = HO.search(cost, start, goal, passable, h0, g_ratio, max_iters, mask, lockstep=True)
            B = cost.shape[0]
            maps = keep[:B]
        else:
            res = HO.search(cost, start, goal, passable, h0, g_ratio, max_iters, mask, lockstep=False)
            maps = keep[:]
    finally:
        HO._Map = saved
    return (res, maps) if with_maps else res


def default_h0(goal) -> np.ndarray:
    """the reference's get_heuristic (Chebyshev + 0.001 Euclidean, fp32 as torch computes it) for [B,H,W] goal maps"""
    goal = np.asarray(goal)
    B, H, W = goal.shape
    out = np.zeros((B, H, W), f32)
    rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for b in range(B):
        g = np.flatnonzero(goal[b].reshape(-1))
        gi = int(g[-1]) if g.size else 0
        dr = np.abs(rr - gi // W).astype(f32)
        dc = np.abs(cc - gi % W).astype(f32)
        cheb = ((dr + dc) - np.minimum(dr, dc)).astype(f32)
        euc = np.sqrt((dr * dr + dc * dc).astype(f32)).astype(f32)
        out[b] = (cheb + (f32(0.001) * euc).astype(f32)).astype(f32)
    return out


# ---- the reference vectors of tools/gen_golden_multisource.py ---------------------------------------------------------------------------
class MGolden(NamedTuple):
    name: str
    mask: int
    g_ratio: float
    Tmax: float
    training: bool
    map_designs: np.ndarray  # [B,1,H,W] f32
    start_maps: np.ndarray   # multi-hot
    goal_maps: np.ndarray
    cost_maps: np.ndarray
    h0: Optional[np.ndarray]  # [B,1,H,W] f32 or None (the reference's heuristic)
    histories: np.ndarray
    paths: np.ndarray
    sel_log: np.ndarray      # [B, t_batch + 1]
    t_batch: int
    target: Optional[np.ndarray]
    grad_cost: Optional[np.ndarray]
    grad_h0: Optional[np.ndarray]
    h0_only: bool
    alone_histories: Optional[np.ndarray]  # coupled vectors: every map searched alone
    alone_paths: Optional[np.ndarray]
    tried: int               # seeds tried / rejected while this vector was generated
    rejected: int

    @property
    def max_iters(self) -> int:
        W = self.map_designs.shape[-1]
        return int((self.Tmax if self.training else 1.0) * W * W)


def names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(DIR, "*.npz")))


def _unpack(bits, B, H, W):
    return np.unpackbits(bits, axis=-1)[..., :H * W].reshape(bits.shape[:-1] + (1, H, W))


def load(name: str) -> MGolden:
    z = np.load(os.path.join(DIR, name + ".npz"))
    B, H, W = int(z["B"]), int(z["H"]), int(z["W"])
    maps = _unpack(z["map_bits"], B, H, W).astype(f32)
    eye = np.eye(H * W, dtype=f32)
    opt = lambda k, conv=lambda x: x: conv(z[k]) if k in z else None  # noqa: E731
    return MGolden(
        name=name, mask=int(z["mask"]), g_ratio=float(z["g_ratio"]), Tmax=float(z["Tmax"]), training=bool(z["training"]),
        map_designs=maps, start_maps=_unpack(z["start_bits"], B, H, W).astype(f32), goal_maps=eye[z["goal_idx"]].reshape(B, 1, H, W),
        cost_maps=z["cost"].astype(f32) if "cost" in z else maps, h0=opt("h0", lambda x: x.astype(f32).reshape(B, 1, H, W)),
        histories=_unpack(z["hist_bits"], B, H, W).astype(f32), paths=_unpack(z["path_bits"], B, H, W).astype(np.int64),
        sel_log=z["sel_log"], t_batch=int(z["t_batch"]),
        target=opt("target_bits", lambda x: _unpack(x, B, H, W).astype(f32)), grad_cost=opt("grad_cost"), grad_h0=opt("grad_h0"),
        h0_only=bool(z["h0_only"]) if "h0_only" in z else False,
        alone_histories=opt("alone_hist_bits", lambda x: _unpack(x, B, H, W).astype(f32)),
        alone_paths=opt("alone_path_bits", lambda x: _unpack(x, B, H, W).astype(np.int64)),
        tried=int(z["seeds_tried"]), rejected=int(z["seeds_rejected"]),
    )
